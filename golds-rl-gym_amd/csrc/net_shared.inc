// Included by net_conv.hip: exact shared-trunk evaluation of conv1/conv2 and their gradients.
//
// The 10 agent images of one env (get_local_states, reference paac/emulator_runner.py:98-111) share
// channels 0-1 and differ only in the one-hot pixel of channel 2.  conv1 is 8x8/4, so the agents'
// conv1 outputs a1_a = relu(S + delta_a) differ from the shared a1_sh = relu(S) in at most 2x2 pixels
// P_a; conv2 is linear in its input, so
//     z2_a = conv2(a1_sh) + b2 + conv2(a1_a - a1_sh)           (second term: <= 16 (pixel, output) pairs)
// and, for the gradients, with DZ2 = sum over the env's agents of dz2_a,
//     dW2  = patches(a1_sh)^T DZ2 + sum_a sum_pairs (a1_a - a1_sh)[p] (x) dz2_a[o]
//     dS   = relu'(S) . T2(DZ2)  + sum_a (relu'(S+delta_a) - relu'(S))[p] . T2(dz2_a)[p]      (p in P_a)
// where T2 is conv2's transposed convolution.  Same sums as the per-agent evaluation, re-associated:
// conv2, its weight gradient and its data gradient run on n_env instead of 10*n_env images (10x fewer
// FLOPs and 10x fewer operand bytes), plus small exact per-agent corrections.  SURVEY H1.
// (included inside namespace grl)

// conv1 output pixels whose 8x8/4 window contains image pixel (ph, pw): candidate c in 0..3
__device__ __forceinline__ bool conv1_cover(int ph, int pw, int c, int &oy1, int &ox1, int &tap1) {
    oy1 = (ph >> 2) - (c >> 1);
    ox1 = (pw >> 2) - (c & 1);
    const int ky = ph - 4 * oy1, kx = pw - 4 * ox1;
    tap1 = ky * 8 + kx;
    return oy1 >= 0 && oy1 < 20 && ox1 >= 0 && ox1 < 20;
}
// conv2 outputs (4x4/2 over 20x20 -> 9x9) whose window contains conv1 pixel (oy1, ox1): candidate q in 0..3
__device__ __forceinline__ bool conv2_cover(int oy1, int ox1, int q, int &o2, int &tap2) {
    const int oy2 = (oy1 >> 1) - (q >> 1), ox2 = (ox1 >> 1) - (q & 1);
    tap2 = (oy1 - 2 * oy2) * 4 + (ox1 - 2 * ox2);
    o2 = oy2 * 9 + ox2;
    return oy2 >= 0 && oy2 < 9 && ox2 >= 0 && ox2 < 9;
}

// per-agent set-up shared by the forward expansion and the backward correction:
// dlt[c][ci] = (a1_a - a1_sh)[p_c][ci] (0 for an invalid candidate), pairs[c*4+q] = o2 | c<<8 | tap2<<12 or -1,
// pix[c] = conv1 pixel index | tap1 << 16, or -1
__device__ __forceinline__ void agent_setup(const float *__restrict__ sraw_env, const float *__restrict__ w1, int ph, int pw, int tid,
                                            float *dlt, int *pairs, int *pix) {
    if (tid < 128) {
        const int c = tid >> 5, ci = tid & 31;
        int oy1, ox1, tap1;
        float d = 0.f;
        if (conv1_cover(ph, pw, c, oy1, ox1, tap1)) {
            const float s = sraw_env[(oy1 * 20 + ox1) * 32 + ci];
            d = fmaxf(s + w1[(tap1 * 3 + 2) * 32 + ci], 0.f) - fmaxf(s, 0.f);
        }
        dlt[tid] = d;
    } else if (tid < 144) {
        const int k = tid - 128, c = k >> 2, q = k & 3;
        int oy1, ox1, tap1, o2, tap2, v = -1;
        if (conv1_cover(ph, pw, c, oy1, ox1, tap1) && conv2_cover(oy1, ox1, q, o2, tap2)) v = o2 | (c << 8) | (tap2 << 12);
        pairs[k] = v;
    } else if (tid < 148) {
        const int c = tid - 144;
        int oy1, ox1, tap1;
        pix[c] = conv1_cover(ph, pw, c, oy1, ox1, tap1) ? ((oy1 * 20 + ox1) | (tap1 << 16)) : -1;
    }
}

// ---- compact slot rows.  An agent's one-hot reaches nr x nc conv2 outputs (nr, nc in 1..3, from its position alone: the
// valid (conv1 candidate, conv2 candidate) pairs factor into a y part and an x part), 6.25 on average.  Per-slot tensors
// (ulist, d2s, the mask words m2s, the conv3 products, gsl, dza) have one row per REAL slot: row sbase[m] + j for slot j of sample m
// (sbase = exclusive prefix sum of the counts in sample order, sbase[n] = live row count), rowagent[row] = m.
__device__ __forceinline__ int slot_axis_count(int p) {       // distinct conv2 output coordinates reachable from image coordinate p
    unsigned mask = 0;
    for (int c = 0; c < 2; ++c) {
        const int o1 = (p >> 2) - c;
        if (o1 < 0 || o1 >= 20) continue;
        for (int q = 0; q < 2; ++q) {
            const int o2 = (o1 >> 1) - q;
            if (o2 >= 0 && o2 < 9) mask |= 1u << o2;
        }
    }
    return __popc(mask);
}

__global__ __launch_bounds__(256) void slot_count_kernel(const uint8_t *__restrict__ pos, int n, int *__restrict__ sbase, int *__restrict__ blksum) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid;
    int c = 0;
    if (m < n) c = slot_axis_count(pos[(size_t)m * 2]) * slot_axis_count(pos[(size_t)m * 2 + 1]);
    if (m < n) sbase[m] = c;       // count for now; slot_place_kernel turns it into the prefix
    int s = c;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) blksum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void slot_scan_kernel(const int *__restrict__ blksum, int nblocks, int *__restrict__ blkoff, int n,
                                                         int *__restrict__ sbase) {
    __shared__ int wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = tid < nblocks ? blksum[tid] : 0;       // nblocks <= 512
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wtot[w];
    if (tid < nblocks) blkoff[tid] = base + incl - v;
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < 16; ++w) tot += wtot[w];
        sbase[n] = tot;       // live row count
    }
}

__global__ __launch_bounds__(256) void slot_place_kernel(const int *__restrict__ blkoff, int n, int *__restrict__ sbase, int *__restrict__ rowagent) {
    __shared__ int wtot[4];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid, lane = tid & 63, wave = tid >> 6;
    const int c = m < n ? sbase[m] : 0;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int base = blkoff[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wtot[w];
    base += incl - c;
    if (m < n) {
        sbase[m] = base;
        for (int j = 0; j < c; ++j) rowagent[base + j] = m;
    }
}

// ---- the compact slot rows in tap-class order (SlotRowsP / SlotGatherT3P, net_gemm.h).  class of a coordinate v of the touched pixel:
// 0, 1, 2..6, 7, 8 -> live taps {0}, {0,1}, {0,1,2}, {1,2}, {2}; key = class(uy) * 5 + class(ux): a deterministic counting sort of the
// live rows (index order inside a key), then the union of the live-tap masks per 256 sorted rows.
__device__ __forceinline__ int slot_axis_class(int v) { return v == 0 ? 0 : v == 1 ? 1 : v <= 6 ? 2 : v == 7 ? 3 : 4; }
__device__ __forceinline__ unsigned slot_axis_taps(int v) {      // bit t: 0 <= v - t <= 6
    unsigned m = 0;
    for (int t = 0; t < 3; ++t) m |= (v - t >= 0 && v - t <= 6) ? 1u << t : 0u;
    return m;
}
constexpr int SLOT_KEYS = 25, SLOT_SORT_BLOCK = 1024;
__global__ __launch_bounds__(SLOT_SORT_BLOCK) void slot_class_kernel(const signed char *__restrict__ ulist, const int *__restrict__ live,
                                                                    unsigned char *__restrict__ skey, unsigned short *__restrict__ srank,
                                                                    unsigned short *__restrict__ stap, int *__restrict__ blkcnt) {
    constexpr int NW = SLOT_SORT_BLOCK / 64;
    __shared__ int wcnt[NW][SLOT_KEYS];
    const int tid = threadIdx.x, r = blockIdx.x * SLOT_SORT_BLOCK + tid, wave = tid >> 6, lane = tid & 63;
    int key = -1;
    if (r < *live) {
        const int u = ulist[r], uy = u / 9, ux = u - uy * 9;
        key = slot_axis_class(uy) * 5 + slot_axis_class(ux);
        const unsigned ty = slot_axis_taps(uy), tx = slot_axis_taps(ux);
        unsigned m = 0;
        for (int t = 0; t < 3; ++t) m |= ((ty >> t) & 1u) ? tx << (3 * t) : 0u;
        skey[r] = (unsigned char)key;
        stap[r] = (unsigned short)m;
    }
    int rank = 0;
#pragma unroll 5
    for (int k = 0; k < SLOT_KEYS; ++k) {
        const unsigned long long b = __ballot(key == k);
        if (lane == 0) wcnt[wave][k] = __popcll(b);
        if (key == k) rank = __popcll(b & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (key >= 0) {
        for (int w = 0; w < wave; ++w) rank += wcnt[w][key];
        srank[r] = (unsigned short)rank;
    }
    if (tid < SLOT_KEYS) {
        int c = 0;
        for (int w = 0; w < NW; ++w) c += wcnt[w][tid];
        blkcnt[blockIdx.x * SLOT_KEYS + tid] = c;
    }
}

__global__ __launch_bounds__(64) void slot_offsets_kernel(const int *__restrict__ blkcnt, int nblocks, const int *__restrict__ live,
                                                          int *__restrict__ blkoff, int *__restrict__ binbase, int *__restrict__ sperm) {
    __shared__ int total[SLOT_KEYS];
    const int tid = threadIdx.x;
    nblocks = min(nblocks, (*live + SLOT_SORT_BLOCK - 1) / SLOT_SORT_BLOCK);      // the workgroups behind the live count hold nothing
    if (tid < SLOT_KEYS) {
        int run = 0, b = 0;
        for (; b + 8 <= nblocks; b += 8) {
            int c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = blkcnt[(b + i) * SLOT_KEYS + tid];
#pragma unroll
            for (int i = 0; i < 8; ++i) { blkoff[(b + i) * SLOT_KEYS + tid] = run; run += c[i]; }
        }
        for (; b < nblocks; ++b) {
            const int c = blkcnt[b * SLOT_KEYS + tid];
            blkoff[b * SLOT_KEYS + tid] = run;
            run += c;
        }
        total[tid] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int k = 0; k < SLOT_KEYS; ++k) { binbase[k] = o; o += total[k]; }
    }
    // the sorted slots behind the live count, up to the end of their 256-row tile, name no row
    const int n = *live, end = (n + 255) / 256 * 256;
    for (int s = n + tid; s < end; s += 64) sperm[s] = -1;
}

__global__ __launch_bounds__(SLOT_SORT_BLOCK) void slot_sorted_place_kernel(const unsigned char *__restrict__ skey, const unsigned short *__restrict__ srank,
                                                                           const int *__restrict__ live, const int *__restrict__ blkoff,
                                                                           const int *__restrict__ binbase, int *__restrict__ sperm) {
    const int r = blockIdx.x * SLOT_SORT_BLOCK + threadIdx.x;
    if (r >= *live) return;
    const int k = skey[r];
    sperm[binbase[k] + blkoff[blockIdx.x * SLOT_KEYS + k] + srank[r]] = r;
}

__global__ __launch_bounds__(256) void slot_tile_masks_kernel(const int *__restrict__ sperm, const unsigned short *__restrict__ stap,
                                                              const int *__restrict__ live, unsigned *__restrict__ tmask) {
    __shared__ unsigned part[4];
    const int s = blockIdx.x * 256 + threadIdx.x;
    unsigned v = 0;
    if (s < *live) v = stap[sperm[s]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tmask[blockIdx.x] = part[0] | part[1] | part[2] | part[3];
}

// row descriptors of SlotGatherT3P (net_gemm.h): tap (0,0) of compact slot row r inside the patch-compact per-agent dz3
// ([n][5][5][64], window origin org[n]) and its position in the 7x7 map
__global__ void slot_rowdesc_kernel(const int *__restrict__ rowagent, const signed char *__restrict__ ulist, const signed char *__restrict__ org,
                                    const int *__restrict__ live, const int *__restrict__ sperm, int rows, int2 *__restrict__ rowdesc) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;      // sorted position (slot_sort): the descriptor of compact row sperm[s]
    if (s >= rows) return;
    int2 d = make_int2(0, (int)(((unsigned)(-16) << 16) | ((unsigned)(-16) & 0xFFFFu)));
    if (s < *live) {
        const int r = sperm[s];
        const int n = rowagent[r], u = ulist[r], g = org[n];
        const int qy = u / 9, qx = u - qy * 9, oy = g / 3, ox = g - oy * 3;
        const int iy0 = qy - 2, ix0 = qx - 2;
        d.x = n * 1600 + ((iy0 - oy) * 5 + (ix0 - ox)) * 64;
        d.y = (int)(((unsigned)iy0 << 16) | ((unsigned)ix0 & 0xFFFFu));
    }
    rowdesc[s] = d;
}

static int slot_index(grl_net *net, const uint8_t *pos, int n) {
    const int nb = (n + 255) / 256;
    hipStream_t st = net->h->stream;
    hipLaunchKernelGGL(slot_count_kernel, dim3(nb), dim3(256), 0, st, pos, n, net->sbase, net->sblk);
    hipLaunchKernelGGL(slot_scan_kernel, dim3(1), dim3(1024), 0, st, net->sblk, nb, net->sblk + 512, n, net->sbase);
    hipLaunchKernelGGL(slot_place_kernel, dim3(nb), dim3(256), 0, st, net->sblk + 512, n, net->sbase, net->rowagent);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// tap-class order of the compact slot rows (needs ulist: after conv2_prep / expand_conv2, or on the resident ulist)
static int slot_prof(grl_net *net, int n);
static int slot_sort(grl_net *net, int n) {
    const int rows = n * 9, nb = (rows + SLOT_SORT_BLOCK - 1) / SLOT_SORT_BLOCK;
    hipStream_t st = net->h->stream;
    const int *live = net->sbase + n;
    hipLaunchKernelGGL(slot_class_kernel, dim3(nb), dim3(SLOT_SORT_BLOCK), 0, st, net->ulist, live, net->skey, net->srank, net->stap, net->sblkcnt);
    hipLaunchKernelGGL(slot_offsets_kernel, dim3(1), dim3(64), 0, st, net->sblkcnt, nb, live, net->sblkoff, net->sbinbase, net->sperm);
    hipLaunchKernelGGL(slot_sorted_place_kernel, dim3(nb), dim3(SLOT_SORT_BLOCK), 0, st, net->skey, net->srank, live, net->sblkoff, net->sbinbase,
                       net->sperm);
    hipLaunchKernelGGL(slot_tile_masks_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, net->sperm, net->stap, live, net->stmask);
    PAAC_HIP(net, hipGetLastError());
    return slot_prof(net, n);
}
// GEMM profiling pass only: the executed share of the slot GEMMs of the chunk whose lists are bound (freshly sorted or resident)
static int slot_prof(grl_net *net, int n) {
    hipStream_t st = net->h->stream;
    const int *live = net->sbase + n;
    net->sfrac = 1.0;
    if (net->prof_on && net->patch_skip) {      // GEMM profiling pass: the share of the 9 taps the slot GEMMs of this chunk execute (per 256-row tile)
        int nlive = 0;
        PAAC_HIP(net, hipStreamSynchronize(st));
        PAAC_HIP(net, hipMemcpy(&nlive, live, sizeof(int), hipMemcpyDeviceToHost));
        const int nt = (nlive + 255) / 256;
        if (nt > 0) {
            std::vector<unsigned> tm(nt);
            PAAC_HIP(net, hipMemcpy(tm.data(), net->stmask, (size_t)nt * 4, hipMemcpyDeviceToHost));
            double a = 0;
            for (int t = 0; t < nt; ++t) a += __builtin_popcount(tm[t] & 0x1FFu);
            net->sfrac = a / (9.0 * nt);
        }
    }
    return GRL_OK;
}

// a2_a = relu(Z2sh + correction_a) differs from the shared a2sh = relu(Z2sh) only at the <= 9 outputs touched by an
// agent's pairs.  Written per env: a2sh; per (agent, slot): the touched pixel ulist (or -1), its activation
// difference d2 = a2_a[u] - a2sh[u] (the operand of the conv3 corrections) and its ReLU mask a2_a[u] > 0 as one word of 64
// channel bits per compact slot row (m2: the gradient step needs only the sign).
// Persistent workgroups (one per CU, strided over envs) keep all of W2 (128 KB) in LDS: every touched output needs up
// to 4 x 32 rows of it, 1.3 MB per env, which from L2 was the kernel's bound.  The env's 10 agents are set up together
// and all 10 x 9 x 64 touched values are computed in one pass (a wave = the 64 channels of one (agent, slot)).
constexpr size_t EXP2_LDS_BYTES = (size_t)(16 * 32 * 64 + 81 * 64 + 10 * 128) * sizeof(float) + (160 + 40 + 90 + 10 + 10) * sizeof(int);
__global__ __launch_bounds__(1024) void expand_conv2_kernel(const float *__restrict__ sraw, const float *__restrict__ z2sh,
                                                           const uint8_t *__restrict__ pos, const float *__restrict__ w1,
                                                           const float *__restrict__ w2, int nenv, float *__restrict__ a2sh,
                                                           float *__restrict__ d2, unsigned long long *__restrict__ m2, signed char *__restrict__ ulist,
                                                           const int *__restrict__ sbase) {
    extern __shared__ __attribute__((aligned(16))) float elds[];
    float *W = elds, *Z = W + 16 * 32 * 64, *dlt = Z + 81 * 64;
    int *pairs = reinterpret_cast<int *>(dlt + 10 * 128), *pix = pairs + 160, *tl = pix + 40, *tcount = tl + 90, *sb = tcount + 10;
    const int tid = threadIdx.x;
    for (int i = tid; i < 16 * 32 * 16; i += blockDim.x) reinterpret_cast<float4 *>(W)[i] = reinterpret_cast<const float4 *>(w2)[i];
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        for (int i = tid; i < 81 * 16; i += blockDim.x) {
            float4 v = reinterpret_cast<const float4 *>(z2sh + (size_t)env * 5184)[i];
            reinterpret_cast<float4 *>(Z)[i] = v;
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            reinterpret_cast<float4 *>(a2sh + (size_t)env * 5184)[i] = v;
        }
        for (int idx = tid; idx < 10 * 148; idx += blockDim.x) {
            const int a = idx / 148, sub = idx - a * 148;
            const int ph = pos[((size_t)env * 10 + a) * 2], pw = pos[((size_t)env * 10 + a) * 2 + 1];
            agent_setup(sraw + (size_t)env * 12800, w1, ph, pw, sub, dlt + a * 128, pairs + a * 16, pix + a * 4);
        }
        __syncthreads();
        if (tid < 192) {    // lane k = (agent, pair): distinct outputs of each agent's <= 16 pairs, in pair order (<= 9 of them)
            const int k = tid, a = k >> 4, kk = k & 15;
            const int pr = k < 160 ? pairs[k] : -1;
            bool first = pr >= 0;
            for (int j = 0; j < kk; ++j) {
                const int pj = pairs[(a < 10 ? a : 0) * 16 + j];
                first = first && !(pj >= 0 && (pj & 255) == (pr & 255));
            }
            const unsigned long long m = __ballot(first);
            const unsigned bits = (unsigned)(m >> (((tid & 63) >> 4) * 16)) & 0xFFFFu;
            if (first) tl[a * 9 + __popc(bits & ((1u << kk) - 1u))] = pr & 255;
            if (kk == 0 && k < 160) tcount[a] = __popc(bits);
        }
        __syncthreads();
        if (tid < 90 && tid % 9 < tcount[tid / 9]) ulist[sbase[(size_t)env * 10 + tid / 9] + tid % 9] = (signed char)tl[tid];
        if (tid >= 128 && tid < 138) sb[tid - 128] = sbase[(size_t)env * 10 + tid - 128];
        __syncthreads();
        // touched outputs: Z + sum over this output's pairs (in pair order) of (a1_a - a1_sh)[p] . W2[tap]; one wave per
        // (agent, slot), lane = output channel
        const int wave = tid >> 6, lane = tid & 63, nwaves = blockDim.x >> 6;
        for (int it = wave; it < 90; it += nwaves) {
            const int a = it / 9, sl = it - a * 9;
            float act = 0.f, dif = 0.f;
            if (sl < tcount[a]) {
                const int o = tl[it];
                const float z = Z[o * 64 + lane];
                float v = z;
                for (int k = 0; k < 16; ++k) {
                    const int pr = pairs[a * 16 + k];
                    if (pr >= 0 && (pr & 255) == o) {
                        const float4 *d4 = reinterpret_cast<const float4 *>(dlt + a * 128 + ((pr >> 8) & 15) * 32);
                        const float *w = W + (pr >> 12) * 32 * 64 + lane;      // W2[tap2][ci][co]
                        float s = 0.f;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float4 dv = d4[j];
                            s = __builtin_fmaf(dv.x, w[(4 * j) * 64], s);
                            s = __builtin_fmaf(dv.y, w[(4 * j + 1) * 64], s);
                            s = __builtin_fmaf(dv.z, w[(4 * j + 2) * 64], s);
                            s = __builtin_fmaf(dv.w, w[(4 * j + 3) * 64], s);
                        }
                        v += s;
                    }
                }
                act = fmaxf(v, 0.f);
                dif = act - fmaxf(z, 0.f);
            }
            const unsigned long long bits = __ballot(act > 0.f);      // the wave = the 64 channels of this (agent, slot)
            if (sl < tcount[a]) {      // compact row of (agent, slot)
                d2[((size_t)sb[a] + sl) * 64 + lane] = dif;
                if (lane == 0) m2[(size_t)sb[a] + sl] = bits;
            }
        }
    }
}

// the per-agent a2 tensor (debug/test access only): the env's shared image with the agent's touched pixels replaced
__global__ __launch_bounds__(256) void materialize_a2_kernel(const float *__restrict__ a2sh, const float *__restrict__ d2,
                                                             const unsigned long long *__restrict__ m2, const signed char *__restrict__ ulist,
                                                             const int *__restrict__ sbase, float *__restrict__ a2) {
    const size_t m = blockIdx.x;      // agent-sample
    const int tid = threadIdx.x, b = sbase[m], cnt = sbase[m + 1] - b;
    for (int i = tid; i < 81 * 16; i += 256)
        reinterpret_cast<float4 *>(a2 + m * 5184)[i] = reinterpret_cast<const float4 *>(a2sh + (m / 10) * 5184)[i];
    __syncthreads();
    for (int idx = tid; idx < cnt * 64; idx += 256) {
        const int u = ulist[b + (idx >> 6)];
        const size_t i = m * 5184 + u * 64 + (idx & 63);
        const bool on = (m2[b + (idx >> 6)] >> (idx & 63)) & 1ull;
        a2[i] = on ? a2[i] + d2[(size_t)b * 64 + idx] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------ conv2 corrections as a GEMM
// The same corrections as expand_conv2_kernel (kept below as the A/B reference, GRL_NET_EXPAND2=lds), restated as ONE matrix
// product so that W2 is read by MFMA tiles instead of 1.3 MB of LDS traffic per env behind five barriers:
//   * an agent's one-hot at image pixel (ph, pw) changes conv1 at up to 4 candidate pixels c = (cy, cx), oy1 = (ph >> 2) - cy;
//     their conv2 outputs lie in rows {H, H-1, H-2}, H = (ph >> 2) >> 1 (likewise columns): a canonical 3 x 3 grid j = (ry, rx),
//     ry = H - oy2.  Which (candidate, canonical output) pairs exist and which conv2 tap joins them depends only on the parity
//     class g = ((ph >> 2) & 1, (pw >> 2) & 1) of the window: ry = qy + (cy == 1 && py == 0), ky2 = ((py - cy) & 1) + 2 qy, qy in {0,1}.
//   * so with A[m] = [delta_c0 | delta_c1 | delta_c2 | delta_c3] (4 x 32 floats, zero for a candidate outside the map) and
//     B_g[(c, ci)][(j, co)] = W2[ky2][kx2][ci][co] for the class's pairs (zero elsewhere), the per-agent term of z2_a at its canonical
//     output j is (A[m] B_g)[j]: a GEMM over agents sorted by class (M = n, K = 128, N = 576).  Its epilogue (EpiConv2Corr) adds
//     the env's shared pre-activation, applies the ReLU and writes what the rest of the net consumes: the difference to the shared
//     activation per compact slot row and the slot's 64 sign bits.  Canonical outputs outside the 9 x 9 map have no slot (-1).
constexpr int CORR_GROUPS = 4;

// One wave per agent: A row, the agent's compact slot list (distinct conv2 outputs of its pairs, in pair order -- the order every
// other kernel assumes), and the canonical-slot maps of the epilogue.
// mode bit 0: the INDEX part -- ulist, cslot: a function of the agent's position and sbase alone (it may run on the lane's index side
// stream, beside the env-level trunk); bit 1: the DATA part -- the A rows from sraw and the slot rows' pre-fill from z2sh.  3 = both.
__global__ __launch_bounds__(256) void conv2_prep_kernel(const float *__restrict__ sraw, const uint8_t *__restrict__ pos,
                                                         const float *__restrict__ w1, const int *__restrict__ sbase, int n,
                                                         const float *__restrict__ z2sh, float *__restrict__ arow, signed char *__restrict__ ulist,
                                                         int *__restrict__ cslot, float *__restrict__ d2, int mode) {
    __shared__ signed char spix[4][16];      // per wave: the conv2 pixel of each of the agent's slot rows
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= n) return;
    const bool do_index = mode & 1, do_data = mode & 2;
    const int env = m / 10, ph = pos[(size_t)m * 2], pw = pos[(size_t)m * 2 + 1];
    const float *sraw_env = sraw + (size_t)env * 12800;
    if (do_data) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {      // delta of candidate c, channel ci
            const int idx = lane + 64 * h, c = idx >> 5, ci = idx & 31;
            int oy1, ox1, tap1;
            float d = 0.f;
            if (conv1_cover(ph, pw, c, oy1, ox1, tap1)) {
                const float s = sraw_env[(oy1 * 20 + ox1) * 32 + ci];
                d = fmaxf(s + w1[(tap1 * 3 + 2) * 32 + ci], 0.f) - fmaxf(s, 0.f);
            }
            arow[(size_t)m * 128 + idx] = d;
        }
    }
    // (a slot a pair reaches is overwritten below: the wave's stores to one address keep program order)
    if (do_index && lane < 9) cslot[(size_t)m * 9 + lane] = -1;
    // lanes 0..15: pair k = (candidate c, conv2 candidate q)
    const int k = lane & 15, c = k >> 2, q = k & 3;
    int o2 = -1, jcan = -1;
    {
        int oy1, ox1, tap1, o, tap2;
        if (lane < 16 && conv1_cover(ph, pw, c, oy1, ox1, tap1) && conv2_cover(oy1, ox1, q, o, tap2)) {
            o2 = o;
            const int H = (ph >> 2) >> 1, Wc = (pw >> 2) >> 1;
            jcan = (H - o / 9) * 3 + (Wc - o % 9);
        }
    }
    int firstlane = lane;      // the first pair (in pair order) that reaches the same output
    for (int j = 15; j >= 0; --j) {
        const int oj = __shfl(o2, j);
        if (j < lane && oj >= 0 && oj == o2) firstlane = j;
    }
    const bool first = lane < 16 && o2 >= 0 && firstlane == lane;
    const unsigned bits = (unsigned)(__ballot(first) & 0xFFFFull);
    const int rank = __popc(bits & ((1u << (lane & 31)) - 1u));
    const int rank_first = __shfl(rank, firstlane);
    const int base = sbase[m];
    if (do_index && first) ulist[base + rank] = (signed char)o2;
    if (do_index && lane < 16 && o2 >= 0) cslot[(size_t)m * 9 + jcan] = base + rank_first;
    if (!do_data) return;
    // the epilogue of the correction GEMM works in place: slot row <- the env's shared pre-activation of its pixel.  16 lanes per row
    // (16-byte pieces), the agent's <= 9 rows in three passes whose loads are in flight together; the rows' pixels go through a
    // per-wave LDS list (round 4; before: one row per pass, 4-byte pieces, and the pixel of row sl found by peeling sl bits)
    const int count = __popc(bits), wv = threadIdx.x >> 6;
    if (first) spix[wv][rank] = (signed char)o2;
    float4 zv[3];
    int orow[3];
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {
        const int row = ps * 4 + (lane >> 4);
        orow[ps] = row < count ? (int)spix[wv][row] : -1;
        zv[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (orow[ps] >= 0) zv[ps] = *reinterpret_cast<const float4 *>(z2sh + ((size_t)env * 81 + orow[ps]) * 64 + (lane & 15) * 4);
    }
#pragma unroll
    for (int ps = 0; ps < 3; ++ps)
        if (orow[ps] >= 0) *reinterpret_cast<float4 *>(d2 + ((size_t)base + ps * 4 + (lane >> 4)) * 64 + (lane & 15) * 4) = zv[ps];
}

// Bt[g][j*64 + co][c*32 + ci]: the class's conv2 kernel slices (see above); rebuilt whenever the parameters change
__global__ void conv2_corr_weights_kernel(const float *__restrict__ w2, float *__restrict__ bt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= CORR_GROUPS * 576 * 128) return;
    const int kk = i & 127, nn = (i >> 7) % 576, g = i / (576 * 128);
    const int c = kk >> 5, ci = kk & 31, j = nn >> 6, co = nn & 63;
    const int py = g >> 1, px = g & 1, cy = c >> 1, cx = c & 1, ry = j / 3, rx = j - ry * 3;
    const int qy = ry - ((cy == 1 && py == 0) ? 1 : 0), qx = rx - ((cx == 1 && px == 0) ? 1 : 0);
    float v = 0.f;
    if (qy >= 0 && qy <= 1 && qx >= 0 && qx <= 1) {
        const int ky2 = ((py - cy) & 1) + 2 * qy, kx2 = ((px - cx) & 1) + 2 * qx;
        v = w2[((ky2 * 4 + kx2) * 32 + ci) * 64 + co];
    }
    bt[i] = v;
}

// deterministic counting sort of the chunk's agents by parity class into 256-row tiles (as patch_sort, four groups)
__device__ __forceinline__ int corr_group(const uint8_t *__restrict__ pos, int m) {
    return (((pos[(size_t)m * 2] >> 2) & 1) << 1) | ((pos[(size_t)m * 2 + 1] >> 2) & 1);
}
__global__ __launch_bounds__(256) void corr_count_kernel(const uint8_t *__restrict__ pos, int n, int *__restrict__ blkcnt) {
    __shared__ int wcnt[4][CORR_GROUPS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid, wave = tid >> 6, lane = tid & 63;
    const int g = m < n ? corr_group(pos, m) : -1;
#pragma unroll
    for (int k = 0; k < CORR_GROUPS; ++k) {
        const int cnt = __popcll(__ballot(g == k));
        if (lane == 0) wcnt[wave][k] = cnt;
    }
    __syncthreads();
    if (tid < CORR_GROUPS) blkcnt[blockIdx.x * CORR_GROUPS + tid] = wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
}
__global__ __launch_bounds__(256) void corr_offsets_kernel(const int *__restrict__ blkcnt, int nblocks, int ntiles, int *__restrict__ blkoff,
                                                           int *__restrict__ goffp, signed char *__restrict__ tilegroup, int *__restrict__ perm) {
    __shared__ int total[CORR_GROUPS], goff[CORR_GROUPS + 1];
    const int tid = threadIdx.x, k = tid >> 6, lane = tid & 63;      // wave k scans group k
    const int per = (nblocks + 63) / 64, lo = min(nblocks, lane * per), hi = min(nblocks, lo + per);
    int s = 0;
    for (int b = lo; b < hi; ++b) s += blkcnt[b * CORR_GROUPS + k];
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    int run = incl - s;
    for (int b = lo; b < hi; ++b) { blkoff[b * CORR_GROUPS + k] = run; run += blkcnt[b * CORR_GROUPS + k]; }
    if (lane == 63) total[k] = incl;
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int g = 0; g < CORR_GROUPS; ++g) { goff[g] = o; o += (total[g] + 255) / 256 * 256; }
        goff[CORR_GROUPS] = o;
    }
    __syncthreads();
    if (tid <= CORR_GROUPS) goffp[tid] = goff[tid];
    for (int i = tid; i < ntiles; i += 256) {
        int g = -1;
#pragma unroll
        for (int q = 0; q < CORR_GROUPS; ++q) g = (i * 256 >= goff[q] && i * 256 < goff[q + 1]) ? q : g;
        tilegroup[i] = (signed char)g;
    }
    for (int g = 0; g < CORR_GROUPS; ++g)
        for (int sl = goff[g] + total[g] + tid; sl < goff[g + 1]; sl += 256) perm[sl] = -1;
}
__global__ __launch_bounds__(256) void corr_place_kernel(const uint8_t *__restrict__ pos, int n, const int *__restrict__ blkoff,
                                                         const int *__restrict__ goffp, int *__restrict__ perm, int *__restrict__ inv) {
    __shared__ int wcnt[4][CORR_GROUPS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid, wave = tid >> 6, lane = tid & 63;
    const int g = m < n ? corr_group(pos, m) : -1;
    int rank = 0;
#pragma unroll
    for (int k = 0; k < CORR_GROUPS; ++k) {
        const unsigned long long b = __ballot(g == k);
        if (lane == 0) wcnt[wave][k] = __popcll(b);
        if (g == k) rank = __popcll(b & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (g >= 0) {
        for (int w = 0; w < wave; ++w) rank += wcnt[w][g];
        const int slot = goffp[g] + blkoff[blockIdx.x * CORR_GROUPS + g] + rank;
        perm[slot] = m;
        inv[m] = slot;      // the agent's row of the correction GEMM: where its canonical cell block lies (EpiConv2Corr, d2c)
    }
}

// ---- the shared trunk is mostly background: an env's <= 90 bins touch a few of its 400 conv1 pixels, the rest of sraw is b1, and a
// conv2 output whose 4x4 window holds no touched pixel is the same vector for every env.  Three small kernels index that (trunk_index):
//   trunk_mark_kernel   per env the 81-bit mask of affected conv2 outputs and the 100-bit mask of touched 2x2 conv1 pixel blocks (the
//                       rows of conv2's transposed convolution), counts per workgroup of TRUNK_ENVS envs
//   trunk_scan_kernel   exclusive prefix of the counts (one workgroup), live totals
//   trunk_emit_kernel   row lists in (env, bit) order -- a deterministic order: the weight gradient sums over the list
// Forward: conv2 runs over the affected rows plus ONE background row (list entry -1: the synthetic all-b1 image), trunk_fill_kernel
// copies that row's result to the rest.  Backward (net_train.inc): conv2's weight gradient sums the affected rows and adds the
// rank-1 term relu(b1)-patch (x) sum of dz2 over the unaffected rows; conv2's transposed convolution runs over the touched blocks
// only (the only consumers of dS are conv1's weight gradient and the per-agent corrections, both at touched pixels), and conv1's
// bias gradient uses  sum_p m[p] G[p] = m_bg . sum_p G[p] + sum_touched (m[p] - m_bg) G[p],  sum_p T2(DZ2)[p] = (sum_t W2[t]) sum_o DZ2[o].
constexpr int TRUNK_ENVS = 16;
__global__ __launch_bounds__(256) void trunk_mark_kernel(const uint8_t *__restrict__ lbins, const uint8_t *__restrict__ abins,
                                                         const uint8_t *__restrict__ pos, int nenv, unsigned *__restrict__ amask,
                                                         unsigned *__restrict__ bmask, unsigned *__restrict__ cmask, unsigned *__restrict__ nmask,
                                                         int *__restrict__ wgcnt) {
    __shared__ unsigned m[TRUNK_ENVS][3], b[TRUNK_ENVS][4], c3[TRUNK_ENVS][2], nb[TRUNK_ENVS][4];
    const int env0 = blockIdx.x * TRUNK_ENVS, tid = threadIdx.x;
    if (tid < TRUNK_ENVS * 3) (&m[0][0])[tid] = 0;
    if (tid >= 64 && tid < 64 + TRUNK_ENVS * 4) (&b[0][0])[tid - 64] = 0;
    __syncthreads();
    {   // 80 locust bins, 10 agent bins, the 10 agents' own positions: 16 lanes per env collect their bits in registers and OR them
        // across the 16 (as LDS atomics the ~2 000 ORs of an env fell on seven words: 27-43 us for 2 MB of input)
        static_assert(TRUNK_ENVS * 16 == 256, "16 lanes per env");
        const int le = tid >> 4, sub = tid & 15, env = env0 + le;
        unsigned mm[3] = {0u, 0u, 0u}, bb[4] = {0u, 0u, 0u, 0u};
        if (env < nenv)
            for (int p = sub; p < 100; p += 16) {
                const uint8_t *q = p < 80 ? lbins + ((size_t)env * 80 + p) * 2 : p < 90 ? abins + ((size_t)env * 10 + (p - 80)) * 2
                                                                                        : pos + ((size_t)env * 10 + (p - 90)) * 2;
                if (q[0] == 255) continue;
                const int ph = q[0], pw = q[1];
                for (int c = 0; c < 4; ++c) {
                    int oy1, ox1, tap1;
                    if (!conv1_cover(ph, pw, c, oy1, ox1, tap1)) continue;
                    const int blk = (oy1 >> 1) * 10 + (ox1 >> 1);
                    const unsigned bbit = 1u << (blk & 31);
                    const int bw = blk >> 5;
                    bb[0] |= bw == 0 ? bbit : 0u; bb[1] |= bw == 1 ? bbit : 0u; bb[2] |= bw == 2 ? bbit : 0u; bb[3] |= bw == 3 ? bbit : 0u;
                    for (int k = 0; k < 4; ++k) {
                        int o2, tap2;
                        if (!conv2_cover(oy1, ox1, k, o2, tap2)) continue;
                        const unsigned mbit = 1u << (o2 & 31);
                        const int mw = o2 >> 5;
                        mm[0] |= mw == 0 ? mbit : 0u; mm[1] |= mw == 1 ? mbit : 0u; mm[2] |= mw == 2 ? mbit : 0u;
                    }
                }
            }
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) {
#pragma unroll
            for (int w = 0; w < 3; ++w) mm[w] |= __shfl_xor(mm[w], d);
#pragma unroll
            for (int w = 0; w < 4; ++w) bb[w] |= __shfl_xor(bb[w], d);
        }
        if (sub == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w) m[le][w] = mm[w];
#pragma unroll
            for (int w = 0; w < 4; ++w) b[le][w] = bb[w];
        }
    }
    __syncthreads();
    if (tid < TRUNK_ENVS * 2) (&c3[0][0])[tid] = 0;
    if (tid >= 64 && tid < 64 + TRUNK_ENVS * 4) (&nb[0][0])[tid - 64] = 0;
    __syncthreads();
    for (int it = tid; it < TRUNK_ENVS * 81; it += 256) {      // blocks some affected conv2 output's 4 x 4 window reads: where sraw must hold values
        const int le = it / 81, o = it - le * 81;
        if (!((m[le][o >> 5] >> (o & 31)) & 1u)) continue;
        const int oy = o / 9, ox = o - oy * 9;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int blk = (oy + (k >> 1)) * 10 + ox + (k & 1);
            atomicOr(&nb[le][blk >> 5], 1u << (blk & 31));
        }
    }
    for (int it = tid; it < TRUNK_ENVS * 49; it += 256) {      // conv3 outputs (7 x 7) whose 3 x 3 window holds an affected conv2 output: 49 bits
        const int le = it / 49, p = it - le * 49, py = p / 7, px = p - py * 7;
        bool any = false;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int o = (py + t / 3) * 9 + px + t % 3;
            any = any || ((m[le][o >> 5] >> (o & 31)) & 1u);
        }
        if (any) atomicOr(&c3[le][p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    if (tid < TRUNK_ENVS * 3 && env0 + tid / 3 < nenv) amask[(size_t)env0 * 3 + tid] = (&m[0][0])[tid];
    if (tid >= 64 && tid < 64 + TRUNK_ENVS * 4 && env0 + (tid - 64) / 4 < nenv) bmask[(size_t)env0 * 4 + tid - 64] = (&b[0][0])[tid - 64];
    if (tid >= 128 && tid < 128 + TRUNK_ENVS * 2 && env0 + (tid - 128) / 2 < nenv) cmask[(size_t)env0 * 2 + tid - 128] = (&c3[0][0])[tid - 128];
    if (tid >= 192 && tid < 192 + TRUNK_ENVS * 4 && env0 + (tid - 192) / 4 < nenv) nmask[(size_t)env0 * 4 + tid - 192] = (&nb[0][0])[tid - 192] | (&b[0][0])[tid - 192];
    if (tid == 0) {
        int ca = 0, cb = 0, cc = 0;
        for (int le = 0; le < TRUNK_ENVS; ++le) {
            ca += __popc(m[le][0]) + __popc(m[le][1]) + __popc(m[le][2]);
            cb += __popc(b[le][0]) + __popc(b[le][1]) + __popc(b[le][2]) + __popc(b[le][3]);
            cc += __popc(c3[le][0]) + __popc(c3[le][1]);
        }
        wgcnt[blockIdx.x * 3] = ca;
        wgcnt[blockIdx.x * 3 + 1] = cb;
        wgcnt[blockIdx.x * 3 + 2] = cc;
    }
}
// counts[0] = affected conv2 rows, [1] = touched blocks, [2] = affected conv3 rows
__global__ __launch_bounds__(1024) void trunk_scan_kernel(const int *__restrict__ wgcnt, int nwg, int *__restrict__ wgoff, int *__restrict__ counts,
                                                          unsigned *__restrict__ umask) {
    __shared__ int wtot[3][16], carry[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) carry[tid] = 0;
    __syncthreads();
    for (int w0 = 0; w0 < nwg; w0 += 1024) {
        const int w = w0 + tid;
        int v[3], incl[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = w < nwg ? wgcnt[w * 3 + k] : 0;
            incl[k] = v[k];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl[k], d, 64);
                if (lane >= d) incl[k] += o;
            }
            if (lane == 63) wtot[k][wave] = incl[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int base = carry[k];
            for (int x = 0; x < wave; ++x) base += wtot[k][x];
            if (w < nwg) wgoff[w * 3 + k] = base + incl[k] - v[k];
        }
        __syncthreads();
        if (tid < 3) {
            int tot = carry[tid];
            for (int x = 0; x < 16; ++x) tot += wtot[tid][x];
            carry[tid] = tot;
        }
        __syncthreads();
    }
    if (tid < 3) counts[tid] = carry[tid];
    if (tid >= 64 && tid < 66) umask[tid - 64] = 0;      // trunk_emit_kernel ORs the envs' conv3 masks into it
}
__global__ __launch_bounds__(256) void trunk_emit_kernel(const unsigned *__restrict__ amask, const unsigned *__restrict__ bmask,
                                                         const unsigned *__restrict__ cmask, const int *__restrict__ wgoff, int nenv,
                                                         int *__restrict__ rowlist, int *__restrict__ blklist, int *__restrict__ c3list,
                                                         unsigned *__restrict__ umask) {
    __shared__ unsigned m[TRUNK_ENVS][3], b[TRUNK_ENVS][4], c3[TRUNK_ENVS][2];
    __shared__ int ea[TRUNK_ENVS], eb[TRUNK_ENVS], ec[TRUNK_ENVS];
    const int env0 = blockIdx.x * TRUNK_ENVS, tid = threadIdx.x;
    if (tid < TRUNK_ENVS * 3) (&m[0][0])[tid] = env0 + tid / 3 < nenv ? amask[(size_t)env0 * 3 + tid] : 0u;
    if (tid >= 64 && tid < 64 + TRUNK_ENVS * 4) (&b[0][0])[tid - 64] = env0 + (tid - 64) / 4 < nenv ? bmask[(size_t)env0 * 4 + tid - 64] : 0u;
    if (tid >= 128 && tid < 128 + TRUNK_ENVS * 2) (&c3[0][0])[tid - 128] = env0 + (tid - 128) / 2 < nenv ? cmask[(size_t)env0 * 2 + tid - 128] : 0u;
    __syncthreads();
    if (tid >= 64 && tid < 66) {      // the chunk's union of affected conv3 outputs (an OR: order does not matter)
        unsigned w = 0;
        for (int le = 0; le < TRUNK_ENVS; ++le) w |= c3[le][tid - 64];
        if (w) atomicOr(&umask[tid - 64], w);
    }
    if (tid == 0) {
        int oa = wgoff[blockIdx.x * 3], ob = wgoff[blockIdx.x * 3 + 1], oc = wgoff[blockIdx.x * 3 + 2];
        for (int le = 0; le < TRUNK_ENVS; ++le) {
            ea[le] = oa;
            eb[le] = ob;
            ec[le] = oc;
            oa += __popc(m[le][0]) + __popc(m[le][1]) + __popc(m[le][2]);
            ob += __popc(b[le][0]) + __popc(b[le][1]) + __popc(b[le][2]) + __popc(b[le][3]);
            oc += __popc(c3[le][0]) + __popc(c3[le][1]);
        }
    }
    __syncthreads();
    for (int it = tid; it < TRUNK_ENVS * 81; it += 256) {
        const int le = it / 81, o = it - le * 81;
        if (!((m[le][o >> 5] >> (o & 31)) & 1u)) continue;
        int before = __popc(m[le][o >> 5] & ((1u << (o & 31)) - 1u));
        for (int w = 0; w < (o >> 5); ++w) before += __popc(m[le][w]);
        rowlist[ea[le] + before] = (env0 + le) * 81 + o;
    }
    for (int it = tid; it < TRUNK_ENVS * 100; it += 256) {
        const int le = it / 100, o = it - le * 100;
        if (!((b[le][o >> 5] >> (o & 31)) & 1u)) continue;
        int before = __popc(b[le][o >> 5] & ((1u << (o & 31)) - 1u));
        for (int w = 0; w < (o >> 5); ++w) before += __popc(b[le][w]);
        blklist[eb[le] + before] = (env0 + le) * 100 + o;
    }
    for (int it = tid; it < TRUNK_ENVS * 49; it += 256) {
        const int le = it / 49, o = it - le * 49;
        if (!((c3[le][o >> 5] >> (o & 31)) & 1u)) continue;
        int before = __popc(c3[le][o >> 5] & ((1u << (o & 31)) - 1u));
        if (o >> 5) before += __popc(c3[le][0]);
        c3list[ec[le] + before] = (env0 + le) * 49 + o;
    }
}
// bg image = b1 at every pixel (the pre-activation of a pixel no bin touches)
__global__ void trunk_bg_kernel(const float *__restrict__ b1, float *__restrict__ bgimg, int *__restrict__ bglist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 12800) bgimg[i] = b1[i & 31];
    if (i == 0) { bglist[0] = -1; bglist[1] = 1; }      // the one-row list (entry, live count) of the background passes
}
// rows a list GEMM did not compute = the background row's result (float4 per lane, 16 lanes per row); npix rows and nw mask words per
// env.  The first blocks also lay out the next layer's background image (bgimg: pixels x 64 copies of bgsrc) when asked to.
__global__ __launch_bounds__(256) void trunk_fill_kernel(const unsigned *__restrict__ mask, int nw, int npix, const float *__restrict__ bg, int nrows,
                                                         float *__restrict__ dst, const float *__restrict__ bgsrc, float *__restrict__ bgimg, int bgpix,
                                                         const unsigned *__restrict__ need) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = i >> 4, c4 = (i & 15) * 4;
    if (bgimg && row < bgpix) *reinterpret_cast<float4 *>(bgimg + (size_t)row * 64 + c4) = *reinterpret_cast<const float4 *>(bgsrc + c4);
    if (row >= nrows) return;
    const int env = row / npix, o = row - env * npix;
    if (need && !((need[o >> 5] >> (o & 31)) & 1u)) return;      // a pixel no consumer of this chunk reads (chunk-level mask)
    if ((mask[(size_t)env * nw + (o >> 5)] >> (o & 31)) & 1u) return;
    *reinterpret_cast<float4 *>(dst + (size_t)row * 64 + c4) = *reinterpret_cast<const float4 *>(bg + c4);
}
// debug / test access to a3sh in the list form: the pixels outside the chunk's union mask were not written; they hold the background row
__global__ __launch_bounds__(256) void materialize_a3sh_kernel(const unsigned *__restrict__ umask, const float *__restrict__ a3bg, float *__restrict__ a3sh) {
    const int env = blockIdx.x;
    for (int i = threadIdx.x; i < 3136; i += 256) {
        const int p = i >> 6;
        if (!((umask[p >> 5] >> (p & 31)) & 1u)) a3sh[(size_t)env * 3136 + i] = a3bg[i & 63];
    }
}
// debug / test access to sraw in the list form: the pixel blocks conv1 skipped (nobody reads them) get their value, b1
__global__ __launch_bounds__(256) void materialize_sraw_kernel(const unsigned *__restrict__ nmask, const float *__restrict__ b1, float *__restrict__ sraw) {
    const int env = blockIdx.x;
    for (int i = threadIdx.x; i < 12800; i += 256) {
        const int pix = i >> 5, oy = pix / 20, ox = pix - oy * 20, blk = (oy >> 1) * 10 + (ox >> 1);
        if (!((nmask[(size_t)env * 4 + (blk >> 5)] >> (blk & 31)) & 1u)) sraw[(size_t)env * 12800 + i] = b1[i & 31];
    }
}
// ybg[p][j] = sum_c a3bg[c] W_dense1[(p, c)][j]: what a background pixel p of a3sh contributes to dense1's pre-activation (per parameter version)
__global__ __launch_bounds__(256) void trunk_ybg_kernel(const float *__restrict__ a3bg, const float *__restrict__ w, float *__restrict__ ybg) {
    const int p = blockIdx.x >> 1, j = (blockIdx.x & 1) * 256 + threadIdx.x;
    float s = 0.f;
    for (int c = 0; c < 64; ++c) s += a3bg[c] * w[(size_t)(p * 64 + c) * 512 + j];
    ybg[p * 512 + j] = s;
}
// ubias[j] = b[j] + sum over the pixels p outside the union mask of ybg[p][j] (pixel order)
// ... and need2: the conv2 pixels some conv3 output of the union mask reads (3 x 3 windows): what trunk_fill has to fill of a2sh
__global__ __launch_bounds__(256) void trunk_ubias_kernel(const float *__restrict__ b, const float *__restrict__ ybg, const unsigned *__restrict__ umask,
                                                          float *__restrict__ ubias, unsigned *__restrict__ need2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const unsigned u0 = umask[0], u1 = umask[1];
    if (blockIdx.x == 0 && threadIdx.x < 128) {      // one conv2 pixel per lane, the words from ballots (three lanes walking 27 pixels each were 7 of the kernel's 20 us)
        const int o = threadIdx.x, oy = o / 9, ox = o - oy * 9;
        bool any = false;
        if (o < 81)
            for (int t = 0; t < 9; ++t) {
                const int py = oy - t / 3, px = ox - t % 3, p = py * 7 + px;
                if (py >= 0 && py < 7 && px >= 0 && px < 7 && ((p < 32 ? u0 >> p : u1 >> (p - 32)) & 1u)) any = true;
            }
        const unsigned long long bal = __ballot(any);
        if (threadIdx.x == 0) { need2[0] = (unsigned)bal; need2[1] = (unsigned)(bal >> 32); }
        if (threadIdx.x == 64) need2[2] = (unsigned)bal;
    }
    // the 49 candidates are requested together (the masked ones too: a dependent load per term was 29 us for 30 KB), added in pixel order
    float y[49];
#pragma unroll
    for (int p = 0; p < 49; ++p) y[p] = ybg[p * 512 + j];
    float s = b[j];
#pragma unroll
    for (int p = 0; p < 49; ++p)
        if (!((p < 32 ? u0 >> p : u1 >> (p - 32)) & 1u)) s += y[p];
    ubias[j] = s;
}
// ---- the observation's index record (obs_index_kernel): what conv1's backward helpers used to derive from lbins / abins / pos inside
// their full-grid kernels, once per env behind workgroup barriers -- the distinct bins of the two count channels with their counts, bucketed
// by tap class, and the agents' candidate-pixel tables -- built once per backward chunk pass by a small kernel the other lanes' GEMMs hide.
// One WAVE owns an env (four envs per workgroup, no workgroup barrier).  The record is lane scratch; an env's record is kObsWords 32-bit
// words (1 152 B = 9 x 128 B):
//   [0]                 header: listed bins of channel 0 | all listed bins << 8 | nslots << 16
//   [kObsOff ..)        33 bytes: bucket offsets into the list; bucket = channel * 16 + q, q = (h % 4) * 4 + w % 4
//   [kObsList .. +90)   the distinct (channel, bin) pairs, packed h | w << 8 | channel << 16 | count << 20, ordered by (channel, q, lowest
//                       point id): the order conv1_wgrad_shared_kernel adds in
//   [kObsPix .. +40)    agent_ds_kernel's 40 (agent, cover) candidates: pixel | tap << 16, or -1
//   [kObsCslot ..)      40 bytes: the candidate's distinct-pixel slot (255: none)
//   [kObsSlotpix ..)    40 x uint16: pixel of a slot
//   [kObsPm .. +13)     400-bit mask of the conv1 pixels whose 8 x 8 window holds a bin (pixel = oy * 20 + ox)
//   [kObsList2 .. +90)  the same packed entries in (h, channel, w) order: the (ky, c, kx) order the forward adds a window's taps in
//                       (written out a second time rather than as a permutation: the forward then reads one list, not two)
// Equal keys meet in a 128-slot hash table in the wave's own LDS (open addressing; at most 90 keys): count and lowest point id per key
// with LDS atomics, instead of every lane comparing itself with 90 others (that form took 36 us per 8 192 envs, this one 11).  The
// order inside a bucket comes from one bit per listed point id in the bucket's three mask words.
constexpr int kObsWords = 288, kObsOff = 4, kObsList = 16, kObsPix = 112, kObsCslot = 152, kObsSlotpix = 162, kObsPm = 182, kObsList2 = 196;
struct ObsWaveLds {
    unsigned key[128], low[128], cnt[128];      // hash table: key (0xFFFFFFFF: free), lowest id, number of points
    unsigned bm[32][3];                         // per bucket: listed point ids 0..31, 32..63, 64..89
    unsigned off[36];
    unsigned pm[16];
};
// a wave's own LDS words, written by some of its lanes and read by others: the hardware runs a wave's LDS accesses in order
__device__ __forceinline__ void obs_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void obs_hash_clear(ObsWaveLds &L, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) { L.key[lane + 64 * i] = 0xFFFFFFFFu; L.low[lane + 64 * i] = 0xFFFFFFFFu; L.cnt[lane + 64 * i] = 0u; }
}
// the slot of `key` (any value but 0xFFFFFFFF); counts the point and keeps the lowest id.  Lanes of one wave may call it together.
__device__ __forceinline__ int obs_hash_add(ObsWaveLds &L, unsigned key, unsigned id) {
    unsigned s = (key * 2654435761u) >> 25;
    for (int t = 0; t < 128; ++t) {      // (bounded: the table cannot fill)
        const unsigned old = atomicCAS(&L.key[s], 0xFFFFFFFFu, key);
        if (old == 0xFFFFFFFFu || old == key) break;
        s = (s + 1) & 127u;
    }
    atomicAdd(&L.cnt[s], 1u);
    atomicMin(&L.low[s], id);
    return (int)s;
}
// PARTS: 1 = what the forward reads (pm, the second order), 2 = what the backward reads (the first order, the agents' tables), 3 = all
template <int PARTS>
__global__ __launch_bounds__(256) void obs_index_kernel(const uint8_t *__restrict__ lbins, const uint8_t *__restrict__ abins,
                                                        const uint8_t *__restrict__ pos, int nenv, int G, unsigned *__restrict__ rec) {
    __shared__ ObsWaveLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, env = blockIdx.x * 4 + wv;
    if (env >= nenv) return;      // wave-uniform, and no workgroup barrier below
    ObsWaveLds &L = lds[wv];
    unsigned *r = rec + (size_t)env * kObsWords;
    // point `lane` (a locust) and point 64 + lane (locusts 64..79, agents 80..89: lanes 0..25)
    const int id1 = 64 + lane, c1 = id1 >= 80 ? 1 : 0;
    int h0, w0, h1 = 255, w1 = 0, ph = 0, pw = 0;
    {
        const uint8_t *b = lbins + ((size_t)env * 80 + lane) * 2;
        h0 = b[0]; w0 = b[1];
        if (lane < 26) {
            const uint8_t *b1 = c1 ? abins + ((size_t)env * 10 + (id1 - 80)) * 2 : lbins + ((size_t)env * 80 + id1) * 2;
            h1 = b1[0]; w1 = b1[1];
        }
        if (lane < 40) { ph = pos[((size_t)env * 10 + (lane >> 2)) * 2]; pw = pos[((size_t)env * 10 + (lane >> 2)) * 2 + 1]; }
    }
    const bool v0 = h0 != 255, v1 = h1 != 255;
    obs_hash_clear(L, lane);
    (&L.bm[0][0])[lane] = 0u;
    if (lane < 32) (&L.bm[0][0])[64 + lane] = 0u;
    if (lane >= 48) L.pm[lane - 48] = 0u;
    obs_wave_sync();
    // the lowest point id in a (channel, bin) lists it, with the bin's count
    const int s0 = v0 ? obs_hash_add(L, (unsigned)(h0 * G + w0), (unsigned)lane) : 0;
    const int s1 = v1 ? obs_hash_add(L, (unsigned)((c1 << 16) | (h1 * G + w1)), (unsigned)id1) : 0;
    obs_wave_sync();
    const bool f0 = v0 && L.low[s0] == (unsigned)lane, f1 = v1 && L.low[s1] == (unsigned)id1;
    const int n0 = __popcll(__ballot(f0)) + __popcll(__ballot(f1 && !c1)), nall = __popcll(__ballot(f0)) + __popcll(__ballot(f1));
    // touched pixels: the four conv1 outputs whose window holds a listed bin
#pragma unroll
    for (int c = 0; c < (PARTS & 1 ? 4 : 0); ++c) {
        const int oya = (h0 >> 2) - (c >> 1), oxa = (w0 >> 2) - (c & 1), oyb = (h1 >> 2) - (c >> 1), oxb = (w1 >> 2) - (c & 1);
        if (f0 && oya >= 0 && oya < 20 && oxa >= 0 && oxa < 20) atomicOr(&L.pm[(oya * 20 + oxa) >> 5], 1u << ((oya * 20 + oxa) & 31));
        if (f1 && oyb >= 0 && oyb < 20 && oxb >= 0 && oxb < 20) atomicOr(&L.pm[(oyb * 20 + oxb) >> 5], 1u << ((oyb * 20 + oxb) & 31));
    }
    const int k0 = (int)L.cnt[s0], k1 = (int)L.cnt[s1];
    if (PARTS & 2) {
        // first order: bucket (channel, q), inside a bucket by point id
        const int bk0 = (h0 & 3) * 4 + (w0 & 3), bk1 = c1 * 16 + (h1 & 3) * 4 + (w1 & 3);
        if (f0) atomicOr(&L.bm[bk0][lane >> 5], 1u << (lane & 31));
        if (f1) atomicOr(&L.bm[bk1][2], 1u << lane);
        obs_wave_sync();
        int bc = lane < 32 ? __popc(L.bm[lane][0]) + __popc(L.bm[lane][1]) + __popc(L.bm[lane][2]) : 0, incl = bc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane < 33) {      // exclusive prefix: the bucket's offset; lane 32: the total
            L.off[lane] = (unsigned)(incl - bc);
            reinterpret_cast<uint8_t *>(r + kObsOff)[lane] = (uint8_t)(incl - bc);
        }
        obs_wave_sync();
        if (f0) {
            const int at = (int)L.off[bk0] + (lane >= 32 ? __popc(L.bm[bk0][0]) : 0) + __popc(L.bm[bk0][lane >> 5] & ((1u << (lane & 31)) - 1u));
            r[kObsList + at] = (unsigned)(h0 | (w0 << 8) | (k0 << 20));
        }
        if (f1) {
            const int at = (int)L.off[bk1] + __popc(L.bm[bk1][0]) + __popc(L.bm[bk1][1]) + __popc(L.bm[bk1][2] & ((1u << lane) - 1u));
            r[kObsList + at] = (unsigned)(h1 | (w1 << 8) | (c1 << 16) | (k1 << 20));
        }
    }
    const unsigned nlist = (unsigned)(n0 | (nall << 8));
    if (PARTS & 1) {
        obs_wave_sync();
        if (lane < 13) r[kObsPm + lane] = L.pm[lane];
        {   // second order: an entry's place is the number of listed entries with a smaller (h, channel, w); the keys are distinct
            const int q0 = f0 ? (h0 << 9) | w0 : 0x7FFFFFFF, q1 = f1 ? (h1 << 9) | (c1 << 8) | w1 : 0x7FFFFFFF;
            int r0 = 0, r1 = 0;
            for (int j = 0; j < 64; ++j) {
                const int kj = __builtin_amdgcn_readlane(q0, j);
                r0 += kj < q0 ? 1 : 0; r1 += kj < q1 ? 1 : 0;
            }
            for (int j = 0; j < 26; ++j) {
                const int kj = __builtin_amdgcn_readlane(q1, j);
                r0 += kj < q0 ? 1 : 0; r1 += kj < q1 ? 1 : 0;
            }
            if (f0) r[kObsList2 + r0] = (unsigned)(h0 | (w0 << 8) | (k0 << 20));
            if (f1) r[kObsList2 + r1] = (unsigned)(h1 | (w1 << 8) | (c1 << 16) | (k1 << 20));
        }
    }
    if (!(PARTS & 2)) {      // the forward's record: header without the agents' slots
        if (lane == 0) r[0] = nlist;
        return;
    }
    // the 40 (agent, cover) candidate pixels and their distinct-pixel table, in candidate order (as agent_ds_kernel builds them):
    // a pixel's slot is the rank of its first candidate among the first candidates
    int px = -1;
    {
        int oy1, ox1, tap1;
        if (lane < 40 && conv1_cover(ph, pw, lane & 3, oy1, ox1, tap1)) px = (oy1 * 20 + ox1) | (tap1 << 16);
        if (lane < 40) r[kObsPix + lane] = (unsigned)px;
    }
    obs_wave_sync();      // every lane has read the bins' table
    obs_hash_clear(L, lane);
    obs_wave_sync();
    const int sp = px >= 0 ? obs_hash_add(L, (unsigned)(px & 0xFFFF), (unsigned)lane) : 0;
    obs_wave_sync();
    const int firstlane = px >= 0 ? (int)L.low[sp] : lane;
    const bool first = px >= 0 && firstlane == lane;
    const unsigned long long fb = __ballot(first);
    const int rank = __popcll(fb & ((1ull << lane) - 1ull));
    const int slot = __shfl(rank, firstlane);
    if (lane < 40) reinterpret_cast<uint8_t *>(r + kObsCslot)[lane] = (uint8_t)(px >= 0 ? slot : 255);
    if (first) reinterpret_cast<unsigned short *>(r + kObsSlotpix)[rank] = (unsigned short)(px & 0xFFFF);
    if (lane == 0) r[0] = nlist | ((unsigned)__popcll(fb) << 16);
}
static int obs_index(grl_net *net, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv, unsigned *rec, hipStream_t st, int parts) {
    const dim3 g((nenv + 3) / 4), b(256);
    const int G = net->h->cfg.grid_size;
    if (parts == 1) hipLaunchKernelGGL(obs_index_kernel<1>, g, b, 0, st, lb, ab, pos, nenv, G, rec);
    else if (parts == 2) hipLaunchKernelGGL(obs_index_kernel<2>, g, b, 0, st, lb, ab, pos, nenv, G, rec);
    else hipLaunchKernelGGL(obs_index_kernel<3>, g, b, 0, st, lb, ab, pos, nenv, G, rec);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}
// conv1_sparse_shared_kernel (net_conv.hip) from the index record: the touched-pixel mask comes out of the record, and a half wave builds its
// pixel's tap list from the env's (h, channel, w)-sorted entries -- a window test per entry, a ballot, and the list is in (ky, c, kx) order --
// instead of scanning 32 count words of two 84 x 84 byte grids.  The grids (14 KB of LDS), their atomics and the take-back pass are gone,
// and three workgroup barriers per env are left of five.  Same terms in the same order: bit-identical sraw.
__global__ __launch_bounds__(256) void conv1_sparse_indexed_kernel(const unsigned *__restrict__ rec, const float *__restrict__ w1,
                                                                   const float *__restrict__ b1, float *__restrict__ sraw,
                                                                   const unsigned *__restrict__ nmask, int nenv) {
    __shared__ unsigned need[4], pm[13];            // blocks anybody reads (nmask == nullptr: all); touched pixels
    __shared__ float vtab[2][96];                   // count / 80, count / 10 as the reference forms them (float64 division rounded to float32)
    __shared__ unsigned short plist[400];
    __shared__ unsigned short evl[8][128];          // per half wave: the non-zero taps of its pixel, in order
    __shared__ unsigned lst[96];                    // the env's entries in (h, channel, w) order
    __shared__ int ntouched, nlist;
    __shared__ __attribute__((aligned(16))) float wl[64 * 2 * 32];      // the two count channels' kernels [tap][c][co]
    const int tid = threadIdx.x;
    for (int i = tid; i < 64 * 2 * 8; i += 256) {
        const int t = i >> 4, c = (i >> 3) & 1, j = i & 7;
        reinterpret_cast<float4 *>(wl)[i] = *reinterpret_cast<const float4 *>(w1 + (t * 3 + c) * 32 + j * 4);
    }
    if (tid >= 64 && tid < 64 + 81) vtab[0][tid - 64] = (float)((double)(tid - 64) / 80.0);
    if (tid >= 160 && tid < 160 + 11) vtab[1][tid - 160] = (float)((double)(tid - 160) / 10.0);
    // this lane's word of the first env's record; inside the loop: of the next one
    unsigned nword = 0u, nneed = 0xFFFFFFFFu;
    auto fetch = [&](int e) {
        if (e < nenv) {
            const unsigned *r = rec + (size_t)e * kObsWords;
            if (tid < 90) nword = r[kObsList2 + tid];      // (words past the env's count are never used)
            else if (tid >= 96 && tid < 109) nword = r[kObsPm + tid - 96];
            else if (tid == 128) nword = (r[0] >> 8) & 255u;
            if (tid < 4 && nmask) nneed = nmask[(size_t)e * 4 + tid];
        }
    };
    fetch(blockIdx.x);
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();      // the previous env's walk is over (evl, plist, pm, need, lst)
        if (tid < 90) lst[tid] = nword;
        else if (tid >= 96 && tid < 109) pm[tid - 96] = nword;
        else if (tid == 128) nlist = (int)nword;
        if (tid < 4) need[tid] = nmask ? nneed : 0xFFFFFFFFu;
        fetch(env + gridDim.x);
        __syncthreads();
        for (int p = tid; p < 400; p += 256)
            if ((pm[p >> 5] >> (p & 31)) & 1u) {
                int before = __popc(pm[p >> 5] & ((1u << (p & 31)) - 1u));
                for (int w = 0; w < (p >> 5); ++w) before += __popc(pm[w]);
                plist[before] = (unsigned short)p;
            }
        if (tid == 0) {
            int n = 0;
            for (int w = 0; w < 13; ++w) n += __popc(pm[w]);
            ntouched = n;
        }
        // the untouched pixels somebody reads: b1
        float4 *out = reinterpret_cast<float4 *>(sraw + (size_t)env * 12800);
        for (int item = tid; item < 3200; item += 256) {
            const int pix = item >> 3, oy = pix / 20, ox = pix - oy * 20, blk = (oy >> 1) * 10 + (ox >> 1);
            if (!((need[blk >> 5] >> (blk & 31)) & 1u) || ((pm[pix >> 5] >> (pix & 31)) & 1u)) continue;
            out[item] = *reinterpret_cast<const float4 *>(b1 + (item & 7) * 4);
        }
        __syncthreads();
        // A touched pixel gets half a wave, one output channel per lane.  Lane l tests entries l, 32 + l, 64 + l against the pixel's window; the
        // entries inside keep their order, so their places are the set bits below them in the half wave's ballot.
        const int co = tid & 31, hw = tid >> 5, nt = ntouched, n = nlist, sh = (tid & 32);
        unsigned short *ev = evl[hw];
        for (int t = hw; t < ((nt + 7) & ~7); t += 8) {      // whole waves run every round (the ballots)
            const bool live = t < nt;
            const int pix = live ? plist[t] : 0, oy = pix / 20, ox = pix - oy * 20;
            int total = 0;
            for (int i0 = 0; i0 < n; i0 += 32) {
                const int i = i0 + co;
                const unsigned e = i < n ? lst[i] : 0u;
                const int ky = (int)(e & 255u) - 4 * oy, kx = (int)((e >> 8) & 255u) - 4 * ox, c = (int)((e >> 16) & 1u);
                const bool in = live && i < n && (unsigned)ky < 8u && (unsigned)kx < 8u;
                const unsigned m = (unsigned)(__ballot(in) >> sh);
                if (in) ev[total + __popc(m & ((1u << co) - 1u))] = (unsigned short)((((ky * 8 + kx) * 2 + c) << 7) | (e >> 20));      // tap-and-channel row of wl, count
                total += __popc(m);
            }
            obs_wave_sync();      // the half wave's list is read by all its lanes
            float acc = b1[co];
            for (int e = 0; e < total; ++e) {
                const int code = ev[e];
                acc += vtab[(code >> 7) & 1][code & 127] * wl[(code >> 7) * 32 + co];
            }
            if (live) sraw[(size_t)env * 12800 + pix * 32 + co] = acc;
            obs_wave_sync();      // ... before the next pixel's list overwrites it
        }
    }
}
static int conv1_sparse_indexed_grid() {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)conv1_sparse_indexed_kernel, 256, 0) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipGetDeviceProperties(&prop, dev) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return 1024;
    }
    return per_cu * prop.multiProcessorCount;
}
static int trunk_index(grl_net *net, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv) {
    hipStream_t st = net->h->stream;
    const int nwg = (nenv + TRUNK_ENVS - 1) / TRUNK_ENVS;
    hipLaunchKernelGGL(trunk_mark_kernel, dim3(nwg), dim3(256), 0, st, lb, ab, pos, nenv, net->tamask, net->tbmask, net->tcmask, net->tnmask, net->twgcnt);
    hipLaunchKernelGGL(trunk_scan_kernel, dim3(1), dim3(1024), 0, st, net->twgcnt, nwg, net->twgoff, net->trows_n, net->tumask);
    hipLaunchKernelGGL(trunk_emit_kernel, dim3(nwg), dim3(256), 0, st, net->tamask, net->tbmask, net->tcmask, net->twgoff, nenv, net->trowlist,
                       net->tblklist, net->tc3list, net->tumask);
    // dense1's per-env bias under the union mask: b + the background's contribution of the pixels outside it
    hipLaunchKernelGGL(trunk_ubias_kernel, dim3(2), dim3(256), 0, st, net->params + ConvOffsets::d1b, (const float *)net->tybg, (const unsigned *)net->tumask,
                       net->tubias, net->tneed2);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}
// live entries of a trunk list -- read back only while profiling (serialised pass), for the FLOP count; otherwise the upper bound
static double trunk_live(grl_net *net, int which, double upper) {
    if (!net->prof_on) return upper;
    int cnt = 0;
    if (hipStreamSynchronize(net->h->stream) != hipSuccess || hipMemcpy(&cnt, net->trows_n + which, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return upper;
    return (double)cnt;
}

// The background's way through conv2 and conv3, once per parameter version (refresh_transposes) and per arithmetic form: the SAME
// GEMM kernels on a one-row list whose entry -1 names the constant image, so that a filled row holds exactly the bits the layer
// would have computed for it.  tbgz = [z2 | a2], tbgz3 = [z3 | a3] of the background; tbgimg3 = a2 of the background at all 81 pixels.
static int trunk_background(grl_net *net) {
    if (!net->shared_trunk || !net->tbgimg) return GRL_OK;
    hipStream_t st = net->h->stream;
    const float *P = net->params, *PT = net->paramsT;
    hipLaunchKernelGGL(trunk_bg_kernel, dim3(12800 / 256), dim3(256), 0, st, P + ConvOffsets::c1b, net->tbgimg, net->tbglist);
    {
        GatherConv2ReluRows g{net->tbgimg, net->tbglist, net->tbglist + 1, net->tbgimg, 1, 1};
        EpiBiasDualRows e{nullptr, nullptr, 64, P + ConvOffsets::c2b, net->tbglist, net->tbglist + 1, net->tbgz, net->tbgz + 64};
        launch_rowk<128, 64, 4, 1, GatherConv2ReluRows, EpiBiasDualRows>(net, dim3(1, 1), st, g, PT + ConvOffsets::c2w, 512, 64, e);
    }
    hipLaunchKernelGGL(trunk_fill_kernel, dim3((81 * 16 + 255) / 256), dim3(256), 0, st, (const unsigned *)nullptr, 0, 1, (const float *)nullptr, 0,
                       (float *)nullptr, (const float *)(net->tbgz + 64), net->tbgimg3, 81, (const unsigned *)nullptr);
    {
        GatherConv3Rows g{net->tbgimg3, net->tbglist, net->tbglist + 1, net->tbgimg3, 1, 1};
        EpiBiasDualRows e{nullptr, nullptr, 64, P + ConvOffsets::c3b, net->tbglist, net->tbglist + 1, net->tbgz3, net->tbgz3 + 64};
        launch_rowk<256, 64, kW256M, kW256N, GatherConv3Rows, EpiBiasDualRows>(net, dim3(1, 1), st, g, PT + ConvOffsets::c3w, 576, 64, e);
    }
    hipLaunchKernelGGL(trunk_ybg_kernel, dim3(98), dim3(256), 0, st, (const float *)(net->tbgz3 + 64), P + ConvOffsets::d1w, net->tybg);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

static int conv1_sparse_grid() {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)conv1_sparse_shared_kernel, 256, 0) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipGetDeviceProperties(&prop, dev) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return 1024;
    }
    return per_cu * prop.multiProcessorCount;
}
// pixels in the chunk's union mask -- read back only while profiling (FLOP count); otherwise the upper bound
static double trunk_union_pixels(grl_net *net) {
    if (!net->prof_on) return 49.0;
    unsigned u[2] = {0xFFFFFFFFu, 0x1FFFFu};
    if (hipStreamSynchronize(net->h->stream) == hipSuccess) (void)hipMemcpy(u, net->tumask, sizeof(u), hipMemcpyDeviceToHost);
    return (double)(__builtin_popcount(u[0]) + __builtin_popcount(u[1] & 0x1FFFFu));
}
static int patch_sort(grl_net *net, int n);
static bool pitem_gather_on(const grl_net *net);
static int pitem_index(grl_net *net, int n, const uint8_t *pos);
// tail: conv3 + dense1 of this pass follow (forward_conv3_dense1_shared) -- the item sort of the conv3 gather may then ride on the side stream
static int forward_conv12_shared(grl_net *net, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv, bool tail) {
    hipStream_t st = net->h->stream;
    net->pitem_on_side = 0;
    const float *P = net->params, *PT = net->paramsT;
    const int n = nenv * 10;
    const bool trunk = net->expand2_gemm && net->trunk_skip;
    // Everything the per-agent index structures need is the agents' positions: the compact slot lists, the class sort of the conv2
    // corrections, the slot and patch sorts with their tile masks -- 17 launches, each a dependent step of ~5 us + a dispatch gap.  With
    // several chunks per step other lanes hide them; with ONE chunk per step (<= 8 192 envs per GPU: the strong-scaling shard) they are
    // ~150 us of a 1 ms forward on the rollout's critical path.  In such a rollout (side_now, lane 0) they run on the side stream, which
    // sits on another hardware queue than the lane (grl_net_create), while the lane computes the env-level trunk (round 5).  Same kernels, same buffers: the side stream starts behind everything already enqueued on the lane
    // (the previous pass's consumers of those buffers) and the main stream waits for it before the first consumer (conv2_prep's data part).
    const bool side = net->idx_side && net->side_now && net->cur_lane == 0 && net->expand2_gemm && !net->prof_on && net->side_stream[0];
    if (side) PAAC_HIP(net, hipEventRecord(net->ev_side0[net->cur_lane], st));      // what is enqueued on the lane so far: the earlier passes' consumers of the lists
    if (trunk)
        if (int rc = trunk_index(net, lb, ab, pos, nenv)) return rc;
    if (side) PAAC_HIP(net, hipEventRecord(net->ev_side2[net->cur_lane], st));      // the trunk's masks are there: the item sort reads cmask
    // list form: sraw is written where somebody reads it -- the 2 x 2 pixel blocks under the affected conv2 outputs' windows
    static const int hgc1 = conv1_sparse_grid();      // one resident wave of workgroups (they stride over the envs)
    if (net->obs_index) {
        // The record's first consumer is the first kernel of the env-level trunk, so the record is written on the lane itself: the index
        // side stream only starts behind the trunk (below) and would make conv1 wait for an event round trip.  (Every pixel of sraw is the
        // sum of its own window, whatever workgroup computes it: this kernel's grid is its own.)
        static const int hgc1i = conv1_sparse_indexed_grid();
        if (int rc = obs_index(net, lb, ab, pos, nenv, net->obsrec, st, 1)) return rc;
        hipLaunchKernelGGL(conv1_sparse_indexed_kernel, dim3(nenv < hgc1i ? nenv : hgc1i), dim3(256), 0, st, (const unsigned *)net->obsrec, P + ConvOffsets::c1w,
                           P + ConvOffsets::c1b, net->sraw, trunk ? (const unsigned *)net->tnmask : (const unsigned *)nullptr, nenv);
    } else
    hipLaunchKernelGGL(conv1_sparse_shared_kernel, dim3(nenv < hgc1 ? nenv : hgc1), dim3(256), 0, st, lb, ab, P + ConvOffsets::c1w, P + ConvOffsets::c1b,
                       net->h->cfg.grid_size, net->sraw, trunk ? (const unsigned *)net->tnmask : (const unsigned *)nullptr, nenv);
    if (trunk) {      // the affected rows; the rest is the background row (trunk_background), filled
        GatherConv2ReluRows gr{net->sraw, net->trowlist, net->trows_n, net->tbgimg, nenv * 81, 1};
        EpiBiasDualRows e{net->z2sh, net->a2sh, 64, P + ConvOffsets::c2b, net->trowlist, net->trows_n, nullptr, nullptr};
        net->prof_tag_cur = PT_ENV_FWD;
        {
            GemmTimer t(net, 2.0 * trunk_live(net, 0, (double)nenv * 81) * 512 * 64);
            launch_rowk<128, 64, 4, 1, GatherConv2ReluRows, EpiBiasDualRows>(net, dim3(1, (nenv * 81 + 127) / 128), st, gr,
                                                                                      PT + ConvOffsets::c2w, 512, 64, e);
        }
        // z2sh is read at the agents' own conv2 pixels only (conv2_prep_kernel), all of them affected rows: only a2sh is filled
        hipLaunchKernelGGL(trunk_fill_kernel, dim3((nenv * 81 * 16 + 255) / 256), dim3(256), 0, st, (const unsigned *)net->tamask, 3, 81,
                           (const float *)(net->tbgz + 64), nenv * 81, net->a2sh, (const float *)nullptr, (float *)nullptr, 0,
                           (const unsigned *)net->tneed2);      // ... and of a2sh only what conv3's windows over the chunk's union mask reach
    } else {
        GatherConv2Relu g{net->sraw, nenv * 81};
        net->prof_tag_cur = PT_ENV_FWD;
        GemmTimer t(net, 2.0 * nenv * 81 * 512 * 64);
        if (net->expand2_gemm) {      // the GEMM path consumes a2sh = relu(z2sh) straight from this epilogue
            EpiBiasDual e{net->z2sh, net->a2sh, 64, P + ConvOffsets::c2b};
            launch_rowk<256, 64, kW256M, kW256N, GatherConv2Relu, EpiBiasDual>(net, dim3(1, (nenv * 81 + 255) / 256), st, g, PT + ConvOffsets::c2w, 512, 64, e);
        } else {
            EpiBiasAct e{net->z2sh, 64, P + ConvOffsets::c2b, ACT_NONE};
            launch_rowk<256, 64, kW256M, kW256N, GatherConv2Relu, EpiBiasAct>(net, dim3(1, (nenv * 81 + 255) / 256), st, g, PT + ConvOffsets::c2w, 512, 64, e);
        }
    }
    if (side) {      // (enqueued behind the trunk's kernels: the queues are served in the order their work arrives)
        hipStream_t ss = net->side_stream[net->cur_lane];
        PAAC_HIP(net, hipStreamWaitEvent(ss, net->ev_side0[net->cur_lane], 0));
        StreamScope on_side(net->h, ss);      // slot_index / patch_sort enqueue on the handle's current stream; every way out of this block puts st back
        int rc = slot_index(net, pos, n);
        if (rc == GRL_OK) {
            const int nb = (n + 255) / 256;
            hipLaunchKernelGGL(conv2_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, ss, net->sraw, pos, P + ConvOffsets::c1w, net->sbase, n, net->z2sh,
                               net->carow, net->ulist, net->cslot, net->d2s, 1);
            hipLaunchKernelGGL(corr_count_kernel, dim3(nb), dim3(256), 0, ss, pos, n, net->cblkcnt);
            hipLaunchKernelGGL(corr_offsets_kernel, dim3(1), dim3(256), 0, ss, net->cblkcnt, nb, net->ctiles, net->cblkoff, net->cgoff, net->ctilegroup,
                               net->cperm);
            hipLaunchKernelGGL(corr_place_kernel, dim3(nb), dim3(256), 0, ss, pos, n, net->cblkoff, net->cgoff, net->cperm, net->cinv);
            rc = patch_sort(net, n);
            if (rc == GRL_OK && tail && pitem_gather_on(net)) {      // the conv3 gather's item sort rides along (needs the trunk's cmask: ev_side2)
                PAAC_HIP(net, hipStreamWaitEvent(ss, net->ev_side2[net->cur_lane], 0));
                rc = pitem_index(net, n, pos);
                net->pitem_on_side = rc == GRL_OK;
            }
        }
        if (rc) return rc;
    }
    if (side) {      // the main stream goes on when the side stream's lists are there
        PAAC_HIP(net, hipEventRecord(net->ev_side1[net->cur_lane], net->side_stream[net->cur_lane]));
        PAAC_HIP(net, hipStreamWaitEvent(st, net->ev_side1[net->cur_lane], 0));
    } else if (int rc = slot_index(net, pos, n)) return rc;
    if (net->expand2_gemm) {
        const int nb = (n + 255) / 256;
        hipLaunchKernelGGL(conv2_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, st, net->sraw, pos, P + ConvOffsets::c1w, net->sbase, n, net->z2sh,
                           net->carow, net->ulist, net->cslot, net->d2s, side ? 2 : 3);
        if (!side) {
        hipLaunchKernelGGL(corr_count_kernel, dim3(nb), dim3(256), 0, st, pos, n, net->cblkcnt);
        hipLaunchKernelGGL(corr_offsets_kernel, dim3(1), dim3(256), 0, st, net->cblkcnt, nb, net->ctiles, net->cblkoff, net->cgoff, net->ctilegroup,
                           net->cperm);
        hipLaunchKernelGGL(corr_place_kernel, dim3(nb), dim3(256), 0, st, pos, n, net->cblkoff, net->cgoff, net->cperm, net->cinv);
        }
        CorrRows g{net->carow, net->cperm, net->ctilegroup, net->ctiles * 256};
        EpiConv2Corr e{net->d2s, net->m2s, net->cperm, net->cslot, net->expand3_gather && net->chunk <= (1u << 17) ? net->a2 : nullptr};
        net->prof_tag_cur = PT_CLASS_CORR;
        GemmTimer t(net, 2.0 * n * 128 * 576 * (6.25 / 9.0));      // the classes have 4, 6, 6 and 9 of the nine outputs (CorrRows::n_ok): 6.25 on average
        launch_rowk<128, 64, 4, 1, CorrRows, EpiConv2Corr, true, true, 1, true>(net, dim3(576 / 64, net->ctiles * 2), st, g, net->w2corr, 128, 576, e);
    } else {
        hipLaunchKernelGGL(expand_conv2_kernel, dim3(nenv < 256 ? nenv : 256), dim3(1024), EXP2_LDS_BYTES, st, net->sraw, net->z2sh, pos,
                           P + ConvOffsets::c1w, P + ConvOffsets::c2w, nenv, net->a2sh, net->d2s, net->m2s, net->ulist, net->sbase);
    }
    PAAC_HIP(net, hipGetLastError());
    return side ? GRL_OK : patch_sort(net, n);
}

// ------------------------------------------------------------------------------------------ backward pieces
// dst[e] = sum of the env's 10 agents' images (per4 float4 each), agents in order
__global__ void reduce_agents_kernel(const float *__restrict__ src, int nenv, int per4, float *__restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // float4 index
    if (i >= (size_t)nenv * per4) return;
    const size_t e = i / per4, r = i - e * per4;
    float4 v[10];
#pragma unroll
    for (int a = 0; a < 10; ++a) v[a] = reinterpret_cast<const float4 *>(src)[(e * 10 + a) * per4 + r];
    float4 s = v[0];
#pragma unroll
    for (int a = 1; a < 10; ++a) { s.x += v[a].x; s.y += v[a].y; s.z += v[a].z; s.w += v[a].w; }
    reinterpret_cast<float4 *>(dst)[i] = s;
}

// conv2-level gradients of the shared-conv3 split.  On entry dz2[e] = relu'(Z2sh) . T3(DZ3)[e] (all agents, shared
// mask) and gsl[(agent, slot)] = T3(dz3_a)[u] before any mask.  Per agent and touched pixel u the true contribution is
// relu'(z2_a[u]) . T3(dz3_a)[u]: it goes to dza (the per-agent dz2 rows the conv2/conv1 corrections read) and the
// difference to the shared-mask value is folded into dz2[e][u], agent by agent (two agents may touch one pixel).
// Round 4: a lane owns FOUR consecutive channels of a slot row (16 lanes per row).  The kernel was bound by instruction issue, not by
// bytes or latency (a wave64 VALU instruction holds its SIMD for 4 cycles; ~1 000 instructions per lane and env in the one-channel
// form; hoisting all of an env's loads in front of the fold made it SLOWER, 108 -> 132-143 us, by what the registers cost in
// occupancy): 16-byte loads / stores and a quarter of the index arithmetic, LDS updates and loop trips per element.  An agent's
// <= 9 x 16 lanes fit one pass; the next agent's operands are fetched while the current one is folded.
__global__ __launch_bounds__(256) void agent_dz2_kernel(const float *__restrict__ gsl, const unsigned long long *__restrict__ m2,
                                                        const float *__restrict__ a2sh, const signed char *__restrict__ ulist,
                                                        const int *__restrict__ sbase, int nenv, float *__restrict__ dz2, float *__restrict__ dza,
                                                        float *__restrict__ bsum, const unsigned *__restrict__ amask, int bgsum) {
    __shared__ __attribute__((aligned(16))) float corr[81 * 64];
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);      // channels 4 (tid & 15) .. + 3 of the final dz2 this workgroup writes (conv2's bias gradient)
    __shared__ int ul[90], sb[11], u0[10];      // u0: the agent's first reachable conv2 output (uy0 * 9 + ux0)
    __shared__ unsigned long long mw[90];       // the slots' sign words
    __shared__ unsigned am[3];
    const int tid = threadIdx.x, sl = tid >> 4, c4 = (tid & 15) * 4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        for (int i = tid; i < 81 * 16; i += 256) reinterpret_cast<float4 *>(corr)[i] = zero4;
        if (tid < 11) sb[tid] = sbase[(size_t)env * 10 + tid];
        if (tid >= 64 && tid < 67) am[tid - 64] = amask ? amask[(size_t)env * 3 + tid - 64] : 0xFFFFFFFFu;
        __syncthreads();
        if (tid < 90) {
            const int a = tid / 9, j = tid - a * 9;
            const bool has = j < sb[a + 1] - sb[a];
            ul[tid] = has ? ulist[sb[a] + j] : -1;
            mw[tid] = has ? m2[(size_t)sb[a] + j] : 0ull;
        }
        // the env's dz2 rows, fetched now and used after the fold (a load behind a store to the same tensor would wait for it, and here
        // they overlap the index chain sbase -> ulist -> slot rows)
        float *dz = dz2 + (size_t)env * 5184;
        float4 dzv[6];
        unsigned okm = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = tid + 256 * k, o = i >> 4;      // float4 index; output pixel
            // list form (bgsum): only the affected rows hold a dz2 (their sum; trunk_closed3_kernel adds the closed-form rest)
            const bool ok = i < 81 * 16 && (!bgsum || ((am[o >> 5] >> (o & 31)) & 1u));
            dzv[k] = zero4;
            if (ok) dzv[k] = reinterpret_cast<const float4 *>(dz)[i];
            okm |= ok ? 1u << k : 0u;
        }
        __syncthreads();
        if (tid < 10) {      // the slots of an agent are a full nr x nc rectangle of the 9 x 9 map (nr, nc <= 3)
            int y0 = 99, x0 = 99;
            for (int j = 0; j < 9; ++j) {
                const int u = ul[tid * 9 + j];
                if (u < 0) continue;
                y0 = min(y0, u / 9); x0 = min(x0, u % 9);
            }
            u0[tid] = y0 > 8 ? 0 : y0 * 9 + x0;
        }
        const float *ash = a2sh + (size_t)env * 5184;
        // operands of agent 0; inside the loop: of agent a + 1
        int u = sl < sb[1] - sb[0] ? ul[sl] : -1;
        float4 g = zero4, sv = zero4;      // (an if, not a select between a load and a constant: that one is compiled as a select of ADDRESSES, the constant in scratch)
        if (u >= 0) {
            g = *reinterpret_cast<const float4 *>(gsl + ((size_t)sb[0] + sl) * 64 + c4);
            sv = *reinterpret_cast<const float4 *>(ash + u * 64 + c4);
        }
        __syncthreads();
#pragma unroll      // the next agent's loads are then new registers, not copies that would wait for them
        for (int a = 0; a < 10; ++a) {
            int un = -1;
            float4 gn = zero4, svn = zero4;
            if (a < 9) {
                un = sl < sb[a + 2] - sb[a + 1] ? ul[(a + 1) * 9 + sl] : -1;
                if (un >= 0) {
                    gn = *reinterpret_cast<const float4 *>(gsl + ((size_t)sb[a + 1] + sl) * 64 + c4);
                    svn = *reinterpret_cast<const float4 *>(ash + un * 64 + c4);
                }
            }
            if (u >= 0) {
                const unsigned bits = (unsigned)(mw[a * 9 + sl] >> c4) & 0xFu;
                const float4 outv = make_float4((bits & 1u) ? g.x : 0.f, (bits & 2u) ? g.y : 0.f, (bits & 4u) ? g.z : 0.f, (bits & 8u) ? g.w : 0.f);
                float4 c = *reinterpret_cast<float4 *>(&corr[u * 64 + c4]);
                c.x += outv.x - (sv.x > 0.f ? g.x : 0.f);
                c.y += outv.y - (sv.y > 0.f ? g.y : 0.f);
                c.z += outv.z - (sv.z > 0.f ? g.z : 0.f);
                c.w += outv.w - (sv.w > 0.f ? g.w : 0.f);
                *reinterpret_cast<float4 *>(&corr[u * 64 + c4]) = c;
                // dza is CANONICAL: [sample][sy][sx][64], cell = conv2 output relative to u0; cells the agent does not have are
                // not written: the gather's descriptors carry the slot rectangle (T2SlotGather, net_gemm.h)
                const int cell = (u / 9 - u0[a] / 9) * 3 + (u % 9 - u0[a] % 9);
                *reinterpret_cast<float4 *>(dza + (((size_t)env * 10 + a) * 9 + cell) * 64 + c4) = outv;
            }
            __syncthreads();
            u = un; g = gn; sv = svn;
        }
        // the adds and stores of the env's dz2 rows (their loads went out with the index loads)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = tid + 256 * k;
            if ((okm >> k) & 1u) {
                const float4 c = reinterpret_cast<const float4 *>(corr)[i];
                const float4 v = make_float4(dzv[k].x + c.x, dzv[k].y + c.y, dzv[k].z + c.z, dzv[k].w + c.w);
                reinterpret_cast<float4 *>(dz)[i] = v;
                cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w;
            }
        }
    }
    __syncthreads();      // fold the sixteen lanes per channel quad in lane-group order (corr is free now)
    reinterpret_cast<float4 *>(corr)[tid] = cs;
    __syncthreads();
    if (tid < 64) {
        float t = 0.f;
#pragma unroll
        for (int gq = 0; gq < 16; ++gq) t += corr[(gq * 16 + (tid >> 2)) * 4 + (tid & 3)];
        bsum[(size_t)blockIdx.x * 64 + tid] = t;
    }
}

// The closed-form parts of the trunk's background (one launch per chunk; dzsum = sum of dz2 over ALL rows of the chunk, bgsum = over
// the unaffected rows; both from agent_dz2_kernel):
//   dW2[tap][ci][co] += relu(b1[ci]) * bgsum[co]                       the unaffected rows' patches are relu(b1) at every tap
//   db2[co]          += dzsum[co]
//   db1[ci]          += (b1[ci] > 0) * sum_{tap, co} W2[tap][ci][co] dzsum[co]     (see EpiGradStride2Rows)
// column sums of the live wave tiles an EpiGradRowsSum GEMM wrote (wt wave tiles per bm rows, n columns): kLiveParts partial rows,
// each over a contiguous range of tiles in index order
constexpr int kLiveParts = 16;
__global__ __launch_bounds__(256) void colsum_live_kernel(const float *__restrict__ csum, const int *__restrict__ live_rows, int bm, int wt, int n,
                                                          float *__restrict__ partial) {
    __shared__ float red[256];
    const int c = threadIdx.x & 63, k = threadIdx.x >> 6;      // n == 64
    const int parts = (*live_rows + bm - 1) / bm * wt, per = (parts + kLiveParts - 1) / kLiveParts;
    const int p0 = blockIdx.x * per, p1 = min(parts, p0 + per);
    float s = 0.f;
    // eight rows requested ahead of the adds, which stay in index order (one load -> wait -> add per row was a 324-deep chain of L2
    // round trips at 8 192 interior envs: 56 us for 5 MB)
    for (int p = p0 + k; p < p1; p += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p + 4 * u < p1 ? csum[(long)(p + 4 * u) * n + c] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (p + 4 * u < p1) s += v[u];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 64) partial[blockIdx.x * 64 + c] = (red[c] + red[64 + c]) + (red[128 + c] + red[192 + c]);
}
// The conv2-level sums of a chunk whose conv3 data gradient ran over the affected rows only.  With G = T3(DZ3) (before the mask),
// m the ReLU mask of a2sh and m_bg that of the background row:
//   sum over the unaffected rows of dz2 = m_bg . (sum_all G - sum_affected G),   sum_all G [ci] = sum_{tap, co} W3[tap][ci][co] DZ3sum[co]
// (conv3 is a VALID convolution: every (output, tap) pair lands inside the 9 x 9 map).  In: DZ3sum (t[192..255], the chunk's conv3 bias
// gradient), the affected rows' column sums of G (gpart) and of the final dz2 (t[0..63], from agent_dz2_kernel).  Out: t[64..127] =
// unaffected rows' sum, t[0..63] += it (all rows), gb3 += DZ3sum.
__global__ __launch_bounds__(256) void trunk_closed3_kernel(const float *__restrict__ w3, const float *__restrict__ a2bg, const float *__restrict__ gpart,
                                                            float *__restrict__ t, float *__restrict__ gb3) {
    __shared__ float red[256], dz3s[64];
    const int tid = threadIdx.x, ci = tid & 63, part = tid >> 6;
    if (tid < 64) dz3s[tid] = t[192 + tid];
    __syncthreads();
    float s = 0.f;
    for (int tap = part; tap < 9; tap += 4)
        for (int co = 0; co < 64; ++co) s += w3[(tap * 64 + ci) * 64 + co] * dz3s[co];
    red[tid] = s;
    __syncthreads();
    if (tid < 64) {
        const float all = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
        float aff = 0.f;
        for (int p = 0; p < kLiveParts; ++p) aff += gpart[p * 64 + tid];
        const float bg = a2bg[tid] > 0.f ? all - aff : 0.f;
        t[64 + tid] = bg;
        t[tid] += bg;
        gb3[tid] += dz3s[tid];
    }
}
// dense1's per-env data gradient under the union mask: for a pixel p outside it only the sum over the chunk's envs is ever used,
//   sum_env gsh3[env][p][c] = sum_j G[j] W_dense1[(p, c)][j],   G = sum_env gd1sh[env]   (one workgroup per pixel, 4 lanes per channel)
__global__ __launch_bounds__(256) void trunk_upix_kernel(const float *__restrict__ w, const float *__restrict__ G, const unsigned *__restrict__ umask,
                                                         float *__restrict__ spix) {
    const int p = blockIdx.x, tid = threadIdx.x, c = tid >> 2, part = tid & 3;
    if ((umask[p >> 5] >> (p & 31)) & 1u) {
        if (part == 0) spix[p * 64 + c] = 0.f;
        return;
    }
    const float *row = w + (size_t)(p * 64 + c) * 512 + part * 128;
    float s = 0.f;
    for (int j = 0; j < 128; ++j) s += G[part * 128 + j] * row[j];
    const float s1 = __shfl_xor(s, 1), t = (part & 1) ? s1 + s : s + s1;      // (0+1), (2+3): the same value on both lanes
    const float t2 = __shfl_xor(t, 2);
    if (part == 0) spix[p * 64 + c] = t + t2;
}
// ... added, under the background row's mask, to the two sums agent_dz3_kernel left in t: [128..191] DZ3 over the unaffected pixels
// (rank-1 term of conv3's weight gradient), [192..255] DZ3 over all pixels (conv3's bias gradient, trunk_closed3_kernel)
__global__ __launch_bounds__(64) void trunk_uadd_kernel(const float *__restrict__ spix, const float *__restrict__ a3bg, float *__restrict__ t) {
    const int c = threadIdx.x;
    float s = 0.f;
    for (int p = 0; p < 49; ++p) s += spix[p * 64 + c];
    if (a3bg[c] > 0.f) { t[128 + c] += s; t[192 + c] += s; }
}
// (slab_reduce_umask_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)
// (trunk_closed_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)

// (conv3_corr_add_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)

// ---- conv2-level corrections as GEMMs.  Conv1 pixels fall into four parity classes k = (oy1&1)*2 + (ox1&1); the
// 2x2 candidate pixels of an agent's one-hot hit every class exactly once, and within a class the conv2 taps that
// connect a pixel to its (up to) four conv2 outputs are fixed: (ty,tx) in {0,1}^2 <-> output (oy1>>1 - (1-ty),
// ox1>>1 - (1-tx)), kernel tap (py + 2(1-ty), px + 2(1-tx)) -- the same pixel-parity decomposition the shared T2 GEMM
// uses (w2t).  gather_t2_kernel lays the operands out class-major:
//     at2[k][m][(ty,tx,co)] = dz2_a[o(ty,tx)][co]  (the agent's masked dz2 row from dza, 0 if outside / invalid)
//     dl[k][m][ci]          = (a1_a - a1_sh)[p_k][ci]
// so that  T2(dz2_a)[p_k] = at2[k][m] . w2t[k]^T          (gemm_rowk, N = 32)
// and      dW2[tap(k,ty,tx)][ci][co] += sum_m dl[k][m][ci] * at2[k][m][(ty,tx,co)]   (gemm_tn, then conv2_corr_add).
// One workgroup lays out kT2Agents agents per round (grid-stride): with one agent per workgroup the launch was 81 920 workgroups of
// ~5 KB each and waited 87 % of its wave cycles (round 2); here the 16 dza loads of a thread (4 agents x 4 classes) are all
// requested before the first store, and the dl part uses every thread instead of half a wave.
constexpr int kT2Agents = 64;
// Since round 3 the at2 operand is not written any more: agent_dz2_kernel leaves dza in a canonical 3 x 3 grid per agent and the two
// GEMMs gather their rows from it (T2SlotGather, net_gemm.h); this kernel writes the 8-byte gather descriptor of every (class, agent)
// row -- tap (0, 0) of class k's conv1 pixel is conv2 output ((oy1 >> 1) - 1, (ox1 >> 1) - 1), relative to the agent's first
// reachable output u0, with the agent's nr x nc slot rectangle packed beside it -- and the dl rows.  Rows m in [n, nrows) are padding
// of the last GEMM tile: invalid descriptors.
__global__ __launch_bounds__(256) void gather_t2_kernel(const float *__restrict__ sraw, const uint8_t *__restrict__ pos,
                                                        const signed char *__restrict__ ulist, const int *__restrict__ sbase,
                                                        const float *__restrict__ w1, int n, int npad, int nrows,
                                                        int2 *__restrict__ rowdesc, float *__restrict__ dl) {
    const int tid = threadIdx.x;
    {   // descriptors: a thread per (agent, class)
        const int m = blockIdx.x * kT2Agents + (tid >> 2), k = tid & 3;
        if (m < nrows) {
            int2 d = make_int2(0, 0);      // nr = nc = 0: every tap invalid
            if (m < n) {
                const int sb0 = sbase[m], cnt = sbase[m + 1] - sb0;
                int y0 = 99, x0 = 99, y1 = -1, x1 = -1;
                for (int j = 0; j < cnt; ++j) {
                    const int u = ulist[sb0 + j];
                    y0 = min(y0, u / 9); y1 = max(y1, u / 9);
                    x0 = min(x0, u % 9); x1 = max(x1, u % 9);
                }
                const int ph = pos[(size_t)m * 2], pw = pos[(size_t)m * 2 + 1], py = k >> 1, px = k & 1;
                const int oy1 = (ph >> 2) - (((ph >> 2) - py) & 1), ox1 = (pw >> 2) - (((pw >> 2) - px) & 1);
                if (cnt > 0 && oy1 >= 0 && oy1 < 20 && ox1 >= 0 && ox1 < 20) {
                    const int iy0 = (oy1 >> 1) - 1 - y0, ix0 = (ox1 >> 1) - 1 - x0;
                    d = make_int2(m * 576 + (iy0 * 3 + ix0) * 64,
                                  (int)(((unsigned)iy0 << 16) | ((unsigned)(y1 - y0 + 1) << 12) | ((unsigned)(x1 - x0 + 1) << 8) | ((unsigned)ix0 & 0xFFu)));
                }
            }
            rowdesc[(size_t)k * npad + m] = d;
        }
    }
    // dl: (agent, class, channel) items over all threads
    for (int it = tid; it < kT2Agents * 128; it += 256) {
        const int a = it >> 7, k = (it >> 5) & 3, ci = it & 31, m = blockIdx.x * kT2Agents + a;
        if (m < n) {
            const int ph = pos[(size_t)m * 2], pw = pos[(size_t)m * 2 + 1], py = k >> 1, px = k & 1;
            const int oy1 = (ph >> 2) - (((ph >> 2) - py) & 1), ox1 = (pw >> 2) - (((pw >> 2) - px) & 1);
            float d = 0.f;
            if (oy1 >= 0 && oy1 < 20 && ox1 >= 0 && ox1 < 20) {
                const float sv = sraw[(size_t)(m / 10) * 12800 + (oy1 * 20 + ox1) * 32 + ci];
                const int tap1 = (ph - 4 * oy1) * 8 + (pw - 4 * ox1);
                d = fmaxf(sv + w1[(tap1 * 3 + 2) * 32 + ci], 0.f) - fmaxf(sv, 0.f);
            }
            dl[((size_t)k * npad + m) * 32 + ci] = d;
        }
    }
}

// (conv2_corr_add_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)

// Backward correction, part B: gt holds relu'(S) . T2(DZ2) on entry (the T2 GEMM's epilogue applies the shared mask) and dS on exit.  One workgroup per env (strided):
// all 10 agents are set up together, every (agent, candidate conv1 pixel c, channel ci) item picks its T2(dz2_a)[p][ci]
// from the class-major GEMM output tt; the masked values are then folded, agent by agent (fixed order, LDS only),
// into the one-hot taps of dW1 and a per-pixel correction table that is added to dS with one pass.
// Round 4: the per-agent set-up this kernel shared with the forward (agent_setup: 1 280 conv1 deltas and 160 pair codes per env) was
// computed and never read here -- only the 40 candidate pixels are; the distinct-pixel table is built by the 40 candidate lanes with
// one ballot instead of a 40-step chain on thread 0 behind a 400-entry map; a lane owns four channels (16-byte loads of tt / sraw /
// w1 and of the dS rows, which are fetched as soon as the pixel table is known and added after the fold).
// IDX (agent_ds_indexed_kernel): the candidate and distinct-pixel tables come out of the env's index record (obs_index_kernel) instead of
// a 40-step shuffle chain behind a barrier, and the fold keeps ONE barrier in front of it instead of one per agent: it runs on one wave,
// whose LDS accesses the hardware executes in order, and within one agent the four covers touch four different taps and pixels (cover
// (dy, dx) is pixel (h/4 - dy, w/4 - dx) and tap (h%4 + 4 dy, w%4 + 4 dx)), so no two lanes of a step meet in acc1h or corr.
// Same values, same order of additions; 44 -> 42 us per 8 192-env chunk: the barriers were not what the kernel waits for.
template <bool IDX>
__device__ __forceinline__ void agent_ds_body(const float *__restrict__ sraw, const uint8_t *__restrict__ pos,
                                              const float *__restrict__ tt, int npad, float *__restrict__ gt,
                                              const float *__restrict__ w1, int nenv, float *__restrict__ slab1h,
                                              float *__restrict__ slab1b, const unsigned *__restrict__ rec) {
    __shared__ __attribute__((aligned(16))) float acc1h[64 * 32];
    __shared__ __attribute__((aligned(16))) float tl[10 * 128];        // masked T2 values: [agent][c][ci] for the agent's own mask ...
    __shared__ __attribute__((aligned(16))) float tsh[10 * 128];       // ... and for the shared mask
    __shared__ __attribute__((aligned(16))) float corr[40 * 32];
    __shared__ int pix[40], cslotid[40], slotpix[40], nslots;
    const int tid = threadIdx.x, c4 = (tid & 7) * 4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < 64 * 8; i += 256) reinterpret_cast<float4 *>(acc1h)[i] = zero4;
    // column sums of the corrections this workgroup adds to dS (their share of conv1's bias gradient): a thread always
    // touches channels 4 (tid & 7) .. + 3
    float4 csc = zero4;
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        const float *senv = sraw + (size_t)env * 12800;
        float *genv = gt + (size_t)env * 12800;
        const unsigned *r = IDX ? rec + (size_t)env * kObsWords : nullptr;
        if (IDX) {      // wave 0 keeps its fold's tables in LDS (it alone reads them there); everybody else reads the record
            if (tid < 40) {
                pix[tid] = (int)r[kObsPix + tid];
                const int cs = reinterpret_cast<const uint8_t *>(r + kObsCslot)[tid];
                cslotid[tid] = cs == 255 ? -1 : cs;
            }
        } else if (tid < 64) {      // the 40 (agent, candidate) conv1 pixels and their distinct-pixel table, in candidate order
            int px = -1;
            if (tid < 40) {
                const int a = tid >> 2, c = tid & 3;
                const int ph = pos[((size_t)env * 10 + a) * 2], pw = pos[((size_t)env * 10 + a) * 2 + 1];
                int oy1, ox1, tap1;
                if (conv1_cover(ph, pw, c, oy1, ox1, tap1)) px = (oy1 * 20 + ox1) | (tap1 << 16);
                pix[tid] = px;
            }
            const int p0 = px >= 0 ? (px & 0xFFFF) : -1 - tid;      // invalid candidates match nobody
            int firstlane = tid;
            for (int j = 39; j >= 0; --j) {
                const int pj = __shfl(p0, j);
                if (j < tid && pj == p0) firstlane = j;
            }
            const bool first = tid < 40 && px >= 0 && firstlane == tid;
            const unsigned long long fb = __ballot(first);
            const int rank = __popcll(fb & ((1ull << tid) - 1ull));
            const int slot = __shfl(rank, firstlane);
            if (tid < 40) cslotid[tid] = px >= 0 ? slot : -1;
            if (first) slotpix[rank] = p0;
            if (tid == 0) nslots = __popcll(fb);
        }
        if (!IDX) __syncthreads();
        // the dS rows of the distinct pixels (<= 40 x 8 lanes: two passes), in flight over the item pass and the fold
        const int ns8 = (IDX ? (int)((r[0] >> 16) & 255u) : nslots) * 8;
        int spx[2] = {0, 0};
        float4 gv[2] = {zero4, zero4};
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2) {
            const int i = tid + 256 * r2;
            if (i < ns8) {
                spx[r2] = IDX ? (int)reinterpret_cast<const unsigned short *>(r + kObsSlotpix)[i >> 3] : slotpix[i >> 3];      // (IDX: kept for the write-back)
                gv[r2] = *reinterpret_cast<const float4 *>(genv + spx[r2] * 32 + c4);
            }
        }
        // (agent a, candidate c, four channels) items: 320 lanes, two passes with their loads in flight together
        float4 tv[2], sv[2], wv[2];
        bool on[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int it = tid + 256 * r, ac = it >> 3;      // ac = a * 4 + c
            const int px = it < 320 ? (IDX ? (int)rec[(size_t)env * kObsWords + kObsPix + ac] : pix[ac]) : -1;
            on[r] = px >= 0;
            tv[r] = sv[r] = wv[r] = zero4;
            if (on[r]) {
                const int p0 = px & 0xFFFF, oy1 = p0 / 20, ox1 = p0 - oy1 * 20, cls = (oy1 & 1) * 2 + (ox1 & 1), tap1 = px >> 16;
                tv[r] = *reinterpret_cast<const float4 *>(tt + ((size_t)cls * npad + (size_t)env * 10 + (ac >> 2)) * 32 + c4);
                sv[r] = *reinterpret_cast<const float4 *>(senv + p0 * 32 + c4);
                wv[r] = *reinterpret_cast<const float4 *>(w1 + (tap1 * 3 + 2) * 32 + c4);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int it = tid + 256 * r;
            if (it < 320) {
                const float4 t = tv[r], sx = sv[r], w = wv[r];
                // relu'(S + delta_a) . T2(dz2_a)  and  relu'(S) . T2(dz2_a)
                reinterpret_cast<float4 *>(tl)[it] = make_float4(sx.x + w.x > 0.f ? t.x : 0.f, sx.y + w.y > 0.f ? t.y : 0.f,
                                                                 sx.z + w.z > 0.f ? t.z : 0.f, sx.w + w.w > 0.f ? t.w : 0.f);
                reinterpret_cast<float4 *>(tsh)[it] = make_float4(sx.x > 0.f ? t.x : 0.f, sx.y > 0.f ? t.y : 0.f, sx.z > 0.f ? t.z : 0.f, sx.w > 0.f ? t.w : 0.f);
            }
        }
        for (int i = tid; i < ns8; i += 256) reinterpret_cast<float4 *>(corr)[i] = zero4;
        for (int a = 0; a < 10; ++a) {      // fold in agent order (two agents may share a pixel or a tap)
            if (!IDX || a == 0) __syncthreads();
            else obs_wave_sync();      // keeps the compiler from moving an agent's LDS reads above the previous agent's writes
            if (tid < 32) {
                const int ac = a * 4 + (tid >> 3), px = pix[ac];
                if (px >= 0) {
                    const float4 ta = reinterpret_cast<const float4 *>(tl)[ac * 8 + (tid & 7)], ts = reinterpret_cast<const float4 *>(tsh)[ac * 8 + (tid & 7)];
                    float4 h = reinterpret_cast<float4 *>(acc1h)[(px >> 16) * 8 + (tid & 7)];      // one-hot channel of dW1 (input 1.0)
                    h.x += ta.x; h.y += ta.y; h.z += ta.z; h.w += ta.w;
                    reinterpret_cast<float4 *>(acc1h)[(px >> 16) * 8 + (tid & 7)] = h;
                    float4 c = reinterpret_cast<float4 *>(corr)[cslotid[ac] * 8 + (tid & 7)];
                    c.x += ta.x - ts.x; c.y += ta.y - ts.y; c.z += ta.z - ts.z; c.w += ta.w - ts.w;
                    reinterpret_cast<float4 *>(corr)[cslotid[ac] * 8 + (tid & 7)] = c;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {      // dS correction
            const int i = tid + 256 * r;
            if (i < ns8) {
                const float4 c = reinterpret_cast<const float4 *>(corr)[i];
                *reinterpret_cast<float4 *>(genv + (IDX ? spx[r] : slotpix[i >> 3]) * 32 + c4) = make_float4(gv[r].x + c.x, gv[r].y + c.y, gv[r].z + c.z, gv[r].w + c.w);
                csc.x += c.x; csc.y += c.y; csc.z += c.z; csc.w += c.w;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 64 * 32; i += 256) slab1h[(size_t)blockIdx.x * 64 * 32 + i] = acc1h[i];
    // fold the per-thread sums in thread order (tsh is free now): channel c <- lanes tid & 7 == c >> 2, in the order of tid >> 3
    reinterpret_cast<float4 *>(tsh)[tid] = csc;
    __syncthreads();
    if (tid < 32) {
        float s = 0.f;
        for (int g = 0; g < 32; ++g) s += tsh[(g * 8 + (tid >> 2)) * 4 + (tid & 3)];
        slab1b[(size_t)blockIdx.x * 32 + tid] = s;
    }
}
__global__ __launch_bounds__(256) void agent_ds_kernel(const float *__restrict__ sraw, const uint8_t *__restrict__ pos,
                                                       const float *__restrict__ tt, int npad, float *__restrict__ gt,
                                                       const float *__restrict__ w1, int nenv, float *__restrict__ slab1h,
                                                       float *__restrict__ slab1b) {
    agent_ds_body<false>(sraw, pos, tt, npad, gt, w1, nenv, slab1h, slab1b, nullptr);
}
__global__ __launch_bounds__(256) void agent_ds_indexed_kernel(const float *__restrict__ sraw, const unsigned *__restrict__ rec,
                                                               const float *__restrict__ tt, int npad, float *__restrict__ gt,
                                                               const float *__restrict__ w1, int nenv, float *__restrict__ slab1h,
                                                               float *__restrict__ slab1b) {
    agent_ds_body<true>(sraw, nullptr, tt, npad, gt, w1, nenv, slab1h, slab1b, rec);
}

// (onehot_reduce_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)
