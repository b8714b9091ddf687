// Included by net_conv.hip (inside namespace grl, after net_shared.inc): dense1 and its gradients on the shared a3.
//
// conv3 spreads an agent's <= 3x3 touched conv2 pixels to at most 5x5 of the 7x7 conv3 outputs, so
//     a3_a = a3sh + d3_a,   a3sh = relu(z3sh) per ENV,   d3_a = 0 outside the agent's 5x5 patch,
// and dense1 (3136 -> 512, the largest GEMM of the network) splits into
//     y_a  = (W^T a3sh + b)            once per env          (1/10 of the rows)
//          + W[patch rows]^T d3_a      per agent, K = 1600   (51 % of the reduction length)
// with the same split for the data gradient (per-env all 3136 columns + per-agent 1600 columns) and the weight
// gradient (a3sh^T sum_a gd1_a + per-group d3^T gd1).  The patch origin (oy, ox) in {0,1,2}^2 selects which 1600 rows
// of W an agent multiplies, so samples are sorted by origin ("group") into 256-row tiles (PatchRows, net_gemm.h).

// origin of the 5x5 patch of conv3 outputs reachable from the touched conv2 pixels (rows uy0..uy0+2 -> r in uy0-2..uy0+2), and the
// part of the patch conv3 can make differ from the shared map at all: conv2 rows uy0..uy1 reach conv3 rows max(uy0 - 2, 0) ..
// min(uy1, 6), relative to the origin [ry0, ry1] inside 0..4 (likewise the columns).  Outside that rectangle d3 is an exact zero.
struct PatchShape { int g, ry0, ry1, rx0, rx1; };
__device__ __forceinline__ PatchShape patch_shape(const signed char *__restrict__ ul, int cnt) {
    int uy0 = 9, ux0 = 9, uy1 = -1, ux1 = -1;
    for (int j = 0; j < cnt; ++j) {
        const int u = ul[j], y = u / 9, x = u - y * 9;
        uy0 = min(uy0, y); ux0 = min(ux0, x); uy1 = max(uy1, y); ux1 = max(ux1, x);
    }
    if (uy0 > 8) return PatchShape{0, 0, 4, 0, 4};      // no touched pixel: group 0, nothing claimed about the patch
    const int oy = min(max(uy0 - 2, 0), 2), ox = min(max(ux0 - 2, 0), 2);
    PatchShape p{oy * 3 + ox, max(uy0 - 2, 0) - oy, min(uy1, 6) - oy, max(ux0 - 2, 0) - ox, min(ux1, 6) - ox};
    if (p.ry0 < 0 || p.ry1 > 4 || p.ry0 > p.ry1) { p.ry0 = 0; p.ry1 = 4; }      // cannot happen for a 3x3 footprint; never claim too little
    if (p.rx0 < 0 || p.rx1 > 4 || p.rx0 > p.rx1) { p.rx0 = 0; p.rx1 = 4; }
    return p;
}
// the nine intervals a footprint produces ([0, e] and [b, 4]) get codes 0..8; anything else is widened to the next one that holds it
__device__ __forceinline__ int span_code(int &r0, int &r1) {
    if (r0 == 0) return r1;
    if (r1 == 4) return 4 + r0;
    r0 = 0;      // an inner interval (not produced by the geometry): treat it as [0, r1]
    return r1;
}

// Deterministic counting sort of the chunk's samples by (patch group, column span, row span), three small launches:
//   group:   key[m] = (group * 9 + column code) * 9 + row code, org[m] = group, smask[m] = the 25-bit support of the sample's patch;
//            rank[m] = samples of the same key before m inside its workgroup of 256; blkcnt[b][key] = samples of that key in workgroup b
//   offsets: blkoff[b][key] = exclusive prefix of blkcnt over b; binbase[key] = first slot of the key (keys of a group are contiguous,
//            every group padded to a multiple of 256 slots); goffp[0..9] = group offsets; tilegroup[slot >> 8] = group or -1;
//            padding slots of perm = -1; the weight-gradient slices
//   place:   perm[binbase[key] + blkoff[b][key] + rank[m]] = m      (index order inside every key)
// Sorting by shape inside a group costs nothing in padding and makes the 128-row tiles (nearly) uniform in what they can skip.
constexpr int PATCH_KEYS = 9 * 81;
constexpr int PATCH_SORT_BLOCK = 1024;      // samples per workgroup of the sort (16 waves): the offsets kernel walks n / 1024 workgroups per key
__global__ __launch_bounds__(PATCH_SORT_BLOCK) void patch_group_kernel(const signed char *__restrict__ ulist, const int *__restrict__ sbase, int n,
                                                          signed char *__restrict__ org, unsigned short *__restrict__ key_out,
                                                          unsigned short *__restrict__ rank_out, unsigned *__restrict__ smask,
                                                          int *__restrict__ blkcnt) {
    constexpr int NW = PATCH_SORT_BLOCK / 64;
    __shared__ int wcnt[NW][PATCH_KEYS];
    const int tid = threadIdx.x, m = blockIdx.x * PATCH_SORT_BLOCK + tid, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < NW * PATCH_KEYS; i += PATCH_SORT_BLOCK) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    int key = -1;
    if (m < n) {
        PatchShape p = patch_shape(ulist + sbase[m], sbase[m + 1] - sbase[m]);
        const int cy = span_code(p.ry0, p.ry1), cx = span_code(p.rx0, p.rx1);
        key = (p.g * 9 + cx) * 9 + cy;
        unsigned mask = 0;
        for (int py = p.ry0; py <= p.ry1; ++py) mask |= ((1u << (p.rx1 - p.rx0 + 1)) - 1u) << (py * 5 + p.rx0);
        org[m] = (signed char)p.g;
        smask[m] = mask;
        key_out[m] = (unsigned short)key;
    }
    // rank among the lanes of this wave that hold the same key, one distinct key per round (lane order = index order)
    int rank = 0;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        if (key == k) {
            rank = __popcll(same & ((1ull << lane) - 1ull));
            if (lane == leader) wcnt[wave][k] = __popcll(same);
        }
        todo &= ~same;
    }
    __syncthreads();
    if (key >= 0) {
        for (int w = 0; w < wave; ++w) rank += wcnt[w][key];
        rank_out[m] = (unsigned short)rank;
    }
    for (int k = tid; k < PATCH_KEYS; k += PATCH_SORT_BLOCK) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) c += wcnt[w][k];
        blkcnt[(size_t)blockIdx.x * PATCH_KEYS + k] = c;
    }
}

constexpr int PATCH_SLICE_ROWS = 1024;      // default rows of one weight-gradient slice (gemm_tn grid z); slices never straddle groups
__global__ __launch_bounds__(768) void patch_offsets_kernel(const int *__restrict__ blkcnt, int nblocks, int ntiles, int *__restrict__ blkoff,
                                                            int *__restrict__ goffp, int *__restrict__ binbase, signed char *__restrict__ tilegroup,
                                                            int *__restrict__ perm, int nslices, int *__restrict__ sbeg,
                                                            int *__restrict__ send, int *__restrict__ sgrp, int slice_rows) {
    __shared__ int total[PATCH_KEYS], gtot[9], goff[10], zfirst[9];
    const int tid = threadIdx.x;
    if (tid < PATCH_KEYS) {      // a thread per key walks the workgroups (coalesced across the keys)
        int run = 0, b = 0;
        for (; b + 8 <= nblocks; b += 8) {      // eight loads in flight: the walk is a chain of memory latencies otherwise
            int c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = blkcnt[(size_t)(b + i) * PATCH_KEYS + tid];
#pragma unroll
            for (int i = 0; i < 8; ++i) { blkoff[(size_t)(b + i) * PATCH_KEYS + tid] = run; run += c[i]; }
        }
        for (; b < nblocks; ++b) {
            const int c = blkcnt[(size_t)b * PATCH_KEYS + tid];
            blkoff[(size_t)b * PATCH_KEYS + tid] = run;
            run += c;
        }
        total[tid] = run;
    }
    __syncthreads();
    if (tid < 9) {      // the 81 keys of a group are contiguous: their bases relative to the group's
        int o = 0;
        for (int c = 0; c < 81; ++c) { const int t = total[tid * 81 + c]; total[tid * 81 + c] = o; o += t; }
        gtot[tid] = o;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int g = 0; g < 9; ++g) { goff[g] = o; o += (gtot[g] + 255) / 256 * 256; }
        goff[9] = o;
        int z = 0;
        for (int g = 0; g < 9; ++g) {
            zfirst[g] = z;
            for (int b = goff[g]; b < goff[g] + gtot[g] && z < nslices; b += slice_rows, ++z) {
                sbeg[z] = b;
                send[z] = min(goff[g] + gtot[g], b + slice_rows);
                sgrp[z] = g;
            }
        }
        for (; z < nslices; ++z) { sbeg[z] = 0; send[z] = 0; sgrp[z] = -1; }
    }
    __syncthreads();
    if (tid < 10) goffp[tid] = goff[tid];
    if (tid < 9) goffp[10 + tid] = zfirst[tid];      // first weight-gradient slice of the group (patch_wmask_kernel)
    if (tid < PATCH_KEYS) binbase[tid] = goff[tid / 81] + total[tid];
    for (int i = tid; i < ntiles; i += 768) {
        int g = -1;
#pragma unroll
        for (int q = 0; q < 9; ++q) g = (i * 256 >= goff[q] && i * 256 < goff[q + 1]) ? q : g;
        tilegroup[i] = (signed char)g;
    }
    for (int g = 0; g < 9; ++g)
        for (int sl = goff[g] + gtot[g] + tid; sl < goff[g + 1]; sl += 768) perm[sl] = -1;
}

__global__ __launch_bounds__(PATCH_SORT_BLOCK) void patch_place_kernel(const unsigned short *__restrict__ key, const unsigned short *__restrict__ rank, int n,
                                                          const int *__restrict__ blkoff, const int *__restrict__ binbase, int *__restrict__ perm,
                                                          int *__restrict__ slot_of) {
    const int m = blockIdx.x * PATCH_SORT_BLOCK + threadIdx.x;
    if (m >= n) return;
    const int k = key[m], slot = binbase[k] + blkoff[(size_t)blockIdx.x * PATCH_KEYS + k] + rank[m];
    perm[slot] = m;
    slot_of[m] = slot;
}

// tmask[t] = union of the supports of the 128 sorted rows of tile t (padding rows and tiles: nothing)
__global__ __launch_bounds__(128) void patch_masks_kernel(const int *__restrict__ perm, const signed char *__restrict__ tilegroup,
                                                          const unsigned *__restrict__ smask, unsigned *__restrict__ tmask) {
    __shared__ unsigned part[2];
    int m = -1;
    if (tilegroup[blockIdx.x >> 1] >= 0) m = perm[(size_t)blockIdx.x * 128 + threadIdx.x];      // slots past the last group are never written
    unsigned v = m >= 0 ? smask[m] : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tmask[blockIdx.x] = part[0] | part[1];
}

// a3sh = relu(z3sh) per env; per agent, inside its 5x5 patch only: a3_a = relu(z3sh + corrections), d3 = a3_a - a3sh
// (compact [py][px][c] layout, 1600 floats) and the ReLU mask a3_a > 0 as 25 words of 64 channel bits (m3: the gradient
// step needs only the sign of a3_a -- 200 bytes per sample instead of a second 6 400-byte tensor).  Corrections as in expand_conv3 of the previous design: sum over the agent's
// touched conv2 pixels u and taps t with u - t = r of prod[(agent, slot)][t].
__global__ __launch_bounds__(256) void expand_conv3_patch_kernel(const float *__restrict__ z3sh, const float *__restrict__ prod,
                                                                 const signed char *__restrict__ ulist, const int *__restrict__ sbase,
                                                                 const signed char *__restrict__ org, const unsigned *__restrict__ smask,
                                                                 const unsigned *__restrict__ wmask, float *__restrict__ a3sh,
                                                                 float *__restrict__ d3, unsigned long long *__restrict__ m3,
                                                                 const unsigned *__restrict__ cmask, const float *__restrict__ z3bg,
                                                                 const unsigned *__restrict__ umask) {
    __shared__ __attribute__((aligned(16))) float Z[49 * 64];
    __shared__ int uy[90], ux[90], og[10], sb[11], wcnt[4], nitems;
    __shared__ unsigned sm[10], wm[10];
    __shared__ unsigned short items[250];
    const int env = blockIdx.x, tid = threadIdx.x;
    // list form (cmask): conv3 computed only the env's affected outputs; every other pixel is the background row z3bg
    const unsigned cm0 = cmask ? cmask[(size_t)env * 2] : 0xFFFFFFFFu, cm1 = cmask ? cmask[(size_t)env * 2 + 1] : 0xFFFFFFFFu;
    // umask: the chunk's union of the cmasks -- dense1's per-env GEMMs and agent_dz3 read a3sh inside it only, so the rest is not written
    const unsigned um0 = umask ? umask[0] : 0xFFFFFFFFu, um1 = umask ? umask[1] : 0xFFFFFFFFu;
    for (int i = tid; i < 49 * 16; i += 256) {
        const int p = i >> 4;
        const bool aff = ((p < 32 ? cm0 >> p : cm1 >> (p - 32)) & 1u) != 0;
        float4 v = aff ? reinterpret_cast<const float4 *>(z3sh + (size_t)env * 3136)[i] : reinterpret_cast<const float4 *>(z3bg)[i & 15];
        reinterpret_cast<float4 *>(Z)[i] = v;
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        if ((p < 32 ? um0 >> p : um1 >> (p - 32)) & 1u) reinterpret_cast<float4 *>(a3sh + (size_t)env * 3136)[i] = v;
    }
    if (tid < 11) sb[tid] = sbase[(size_t)env * 10 + tid];
    if (tid >= 128 && tid < 138) {
        const size_t m = (size_t)env * 10 + tid - 128;
        og[tid - 128] = org[m];
        // smask == nullptr (GRL_PATCH_SKIP=off): the whole 5x5 patch of every agent, as before the support masks
        sm[tid - 128] = smask ? smask[m] : 0x1FFFFFFu;
        wm[tid - 128] = wmask ? wmask[m] : 0x1FFFFFFu;
    }
    __syncthreads();
    if (tid < 90) {
        const int a = tid / 9, j = tid - a * 9;
        const int u = j < sb[a + 1] - sb[a] ? ulist[sb[a] + j] : -1;
        uy[tid] = u < 0 ? -100 : u / 9;
        ux[tid] = u < 0 ? -100 : u % 9;
    }
    // the (agent, pixel) items of this env that some GEMM may read (wmask: ~8 of 25 pixels per agent on the bench workload), in
    // (agent, pixel) order: one item per 16 lanes below instead of 25 pixels per agent
    {
        const int a = tid / 25, q = tid - a * 25;
        const bool need = tid < 250 && ((wm[a < 10 ? a : 0] >> q) & 1u);
        const unsigned long long b = __ballot(need);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wcnt[w];
        if (need) items[base + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)((a << 8) | q);
        if (tid == 0) nitems = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    __syncthreads();
    // A lane owns FOUR consecutive channels of a patch pixel (16 lanes per pixel, 4 pixels per wave): the kernel is bound by
    // instruction issue, not by bytes (a wave64 VALU instruction occupies its SIMD for 4 cycles), so 16-byte loads / stores and a
    // quarter of the index arithmetic per element.  The mask word of a pixel (64 channel bits) is assembled from the four
    // component ballots by the pixel's first lane.
    auto spread16 = [](unsigned long long x) {      // bit i of the low 16 -> bit 4 i
        x = (x | (x << 24)) & 0x000000FF000000FFull;
        x = (x | (x << 12)) & 0x000F000F000F000Full;
        x = (x | (x << 6)) & 0x0303030303030303ull;
        x = (x | (x << 3)) & 0x1111111111111111ull;
        return x;
    };
    const int lane = tid & 63, c4 = (tid & 15) * 4, cnt = nitems;
    for (int it0 = 0; it0 < cnt; it0 += 16) {      // whole waves run every pass (the ballots below)
        const int it = it0 + (tid >> 4);
        const bool live = it < cnt;
        const int code = live ? items[it] : 0, a = code >> 8, q = code & 255, py = q / 5, px = q - py * 5;
        const size_t m = (size_t)env * 10 + a;
        const int oy = og[a] / 3, ox = og[a] - oy * 3, ry = oy + py, rx = ox + px;
        const bool inside = live && ((sm[a] >> q) & 1u);      // the agent's own support: elsewhere d3 is zero and nobody reads m3
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f), v = z;
        if (inside) {
            z = *reinterpret_cast<const float4 *>(&Z[(ry * 7 + rx) * 64 + c4]);
            v = z;
            const float *pa = prod + (size_t)sb[a] * 576;      // the agent's compact slot rows
#pragma unroll
            for (int sl = 0; sl < 9; ++sl) {
                const int ty = uy[a * 9 + sl] - ry, tx = ux[a * 9 + sl] - rx;
                if ((unsigned)ty < 3u && (unsigned)tx < 3u) {
                    const float4 p4 = *reinterpret_cast<const float4 *>(pa + sl * 576 + (ty * 3 + tx) * 64 + c4);
                    v.x += p4.x; v.y += p4.y; v.z += p4.z; v.w += p4.w;
                }
            }
        }
        const float4 act = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        if (live)
            *reinterpret_cast<float4 *>(d3 + m * 1600 + (size_t)q * 64 + c4) =
                make_float4(act.x - fmaxf(z.x, 0.f), act.y - fmaxf(z.y, 0.f), act.z - fmaxf(z.z, 0.f), act.w - fmaxf(z.w, 0.f));
        const unsigned long long b0 = __ballot(inside && act.x > 0.f), b1 = __ballot(inside && act.y > 0.f),
                                 b2 = __ballot(inside && act.z > 0.f), b3 = __ballot(inside && act.w > 0.f);
        if (inside && (lane & 15) == 0) {
            const int sh = lane & 48;      // the 16 lanes of this pixel
            m3[m * 25 + q] = spread16((b0 >> sh) & 0xFFFFull) | (spread16((b1 >> sh) & 0xFFFFull) << 1) |
                             (spread16((b2 >> sh) & 0xFFFFull) << 2) | (spread16((b3 >> sh) & 0xFFFFull) << 3);
        }
    }
}

// the per-agent a3 tensor (debug/test access, and the per-agent-mask consumers until they move to the patch form)
__global__ __launch_bounds__(256) void materialize_a3_kernel(const float *__restrict__ a3sh, const float *__restrict__ d3,
                                                             const unsigned long long *__restrict__ m3, const signed char *__restrict__ org,
                                                             const unsigned *__restrict__ smask, float *__restrict__ a3) {
    const size_t m = blockIdx.x;
    const int tid = threadIdx.x, g = org[m], oy = g / 3, ox = g - oy * 3;
    const unsigned sm = smask ? smask[m] : 0x1FFFFFFu;      // outside the support the agent's a3 is the shared one (d3 / m3 are not defined there)
    for (int i = tid; i < 49 * 16; i += 256)
        reinterpret_cast<float4 *>(a3 + m * 3136)[i] = reinterpret_cast<const float4 *>(a3sh + (m / 10) * 3136)[i];
    __syncthreads();
    for (int idx = tid; idx < 1600; idx += 256) {
        const int q = idx >> 6, py = q / 5, px = q - py * 5;
        const size_t i = m * 3136 + ((oy + py) * 7 + ox + px) * 64 + (idx & 63);
        if (!((sm >> q) & 1u)) continue;
        const bool on = (m3[m * 25 + q] >> (idx & 63)) & 1ull;
        a3[i] = on ? a3[i] + d3[m * 1600 + idx] : 0.f;      // a3_a = a3sh + d3 where it is positive
    }
}

// zmask[z] = union over the tiles of weight-gradient slice z (slices are 128-aligned ranges inside one group)
__global__ void patch_slice_masks_kernel(const int *__restrict__ sbeg, const int *__restrict__ send, int nslices, const unsigned *__restrict__ tmask,
                                         unsigned *__restrict__ zmask) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= nslices) return;
    const int b = sbeg[z], e = send[z];
    unsigned m = 0;
    if (b < e)
        for (int t = b >> 7; t <= ((e - 1) >> 7); ++t) m |= tmask[t];
    zmask[z] = m;
}

// wmask[m] = the pixels of sample m's patch that ANY GEMM may read: the union of its weight-gradient slice (a superset of the union of
// its 128-row tile).  expand_conv3_patch_kernel defines d3 exactly there (values inside the sample's own support, zeros around it).
__global__ void patch_wmask_kernel(const int *__restrict__ slot_of, const signed char *__restrict__ org, const int *__restrict__ goffp, int n,
                                   int slice_rows, const unsigned *__restrict__ zmask, unsigned *__restrict__ wmask) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const int g = org[m];
    wmask[m] = zmask[goffp[10 + g] + (slot_of[m] - goffp[g]) / slice_rows];
}

static int patch_prof(grl_net *net);
static int patch_sort(grl_net *net, int n) {
    if (int rc = slot_sort(net, n)) return rc;      // the slot rows' own order (net_shared.inc): same inputs, same call sites
    const int nb = (n + PATCH_SORT_BLOCK - 1) / PATCH_SORT_BLOCK;
    hipStream_t st = net->h->stream;
    hipLaunchKernelGGL(patch_group_kernel, dim3(nb), dim3(PATCH_SORT_BLOCK), 0, st, net->ulist, net->sbase, n, net->org, net->pkey, net->prank, net->smask,
                       net->blkcnt);
    hipLaunchKernelGGL(patch_offsets_kernel, dim3(1), dim3(768), 0, st, net->blkcnt, nb, net->ptiles, net->blkoff, net->goffp, net->binbase,
                       net->tilegroup, net->perm, net->pslices, net->sbeg, net->send, net->sgrp, net->pslice_rows);
    hipLaunchKernelGGL(patch_place_kernel, dim3(nb), dim3(PATCH_SORT_BLOCK), 0, st, net->pkey, net->prank, n, net->blkoff, net->binbase, net->perm, net->slot_of);
    hipLaunchKernelGGL(patch_masks_kernel, dim3(net->ptiles * 2), dim3(128), 0, st, net->perm, net->tilegroup, net->smask, net->tmask);
    hipLaunchKernelGGL(patch_slice_masks_kernel, dim3((net->pslices + 127) / 128), dim3(128), 0, st, net->sbeg, net->send, net->pslices, net->tmask, net->zmask);
    hipLaunchKernelGGL(patch_wmask_kernel, dim3((n + 255) / 256), dim3(256), 0, st, net->slot_of, net->org, net->goffp, n, net->pslice_rows, net->zmask, net->wmask);
    PAAC_HIP(net, hipGetLastError());
    return patch_prof(net);
}
// GEMM profiling pass only: the executed share of the dense1 patch GEMMs of the chunk whose lists are bound (freshly sorted or resident)
static int patch_prof(grl_net *net) {
    hipStream_t st = net->h->stream;
    net->pfrac[0] = net->pfrac[1] = net->pfrac[2] = 1.0;
    if (net->prof_on && net->patch_skip) {
        // GEMM profiling pass (single stream): which share of the 25 patch pixels the three dense1 patch GEMMs of this chunk execute,
        // so that their FLOP counts are those of the work done -- forward per 128-row tile, data gradient per 256-row tile, weight
        // gradient per slice
        std::vector<unsigned> tm((size_t)net->ptiles * 2);
        std::vector<int> sb(net->pslices), se(net->pslices);
        PAAC_HIP(net, hipStreamSynchronize(st));
        PAAC_HIP(net, hipMemcpy(tm.data(), net->tmask, tm.size() * 4, hipMemcpyDeviceToHost));
        PAAC_HIP(net, hipMemcpy(sb.data(), net->sbeg, sb.size() * 4, hipMemcpyDeviceToHost));
        PAAC_HIP(net, hipMemcpy(se.data(), net->send, se.size() * 4, hipMemcpyDeviceToHost));
        double a0 = 0, t0 = 0, a1 = 0, t1 = 0, a2 = 0, t2 = 0;
        for (size_t t = 0; t < tm.size(); ++t)
            if (tm[t]) { a0 += __builtin_popcount(tm[t]); t0 += 25; }
        // (the pair forms multiply whole 128-wide tiles: an odd number of live pixels executes one pixel more than is live)
        if (net->pdgrad_pair) {
            for (size_t t = 0; t < tm.size(); ++t)
                if (tm[t]) { a1 += (__builtin_popcount(tm[t]) + 1) / 2 * 2; t1 += 25; }
        } else
        for (size_t t = 0; t + 1 < tm.size(); t += 2)
            if (tm[t] | tm[t + 1]) { a1 += __builtin_popcount(tm[t] | tm[t + 1]); t1 += 25; }
        for (int z = 0; z < net->pslices; ++z) {
            if (se[z] <= sb[z]) continue;
            unsigned m = 0;
            for (int t = sb[z] >> 7; t <= ((se[z] - 1) >> 7); ++t) m |= tm[t];
            a2 += (double)(se[z] - sb[z]) * (net->pwgrad_pair ? (__builtin_popcount(m) + 1) / 2 * 2 : __builtin_popcount(m));
            t2 += (double)(se[z] - sb[z]) * 25;
        }
        if (t0 > 0) net->pfrac[0] = a0 / t0;
        if (t1 > 0) net->pfrac[1] = a1 / t1;
        if (t2 > 0) net->pfrac[2] = a2 / t2;
    }
    return GRL_OK;
}

// ------------------------------------------------------------------------------------------ conv3's corrections gathered at the patch pixels
// (round 4; SlotsToPatch / EpiPatchExpand in net_gemm.h).  What this path needs beside the GEMM:
//   a3sh_relu_kernel     a3sh = relu(z3sh) per env under the chunk's union mask (the first loop of expand_conv3_patch_kernel)
//   (d2c, the agents' touched conv2 pixels as canonical 3 x 3 cell blocks [row][jy][jx][64], is a second output of EpiConv2Corr)
//   pitem_*              the (sample, patch pixel) items of wmask as GEMM rows sorted by their SET OF LIVE TAPS (a counting sort over
//                        64 keys with LDS histograms / cursors per 256 samples: a 128-row tile then multiplies exactly the taps its
//                        rows have), their gather descriptors and the tiles' tap masks
__global__ __launch_bounds__(256) void a3sh_relu_kernel(const float *__restrict__ z3sh, const unsigned *__restrict__ cmask,
                                                        const float *__restrict__ z3bg, const unsigned *__restrict__ umask,
                                                        float *__restrict__ a3sh) {
    const int env = blockIdx.x, tid = threadIdx.x;
    const unsigned cm0 = cmask ? cmask[(size_t)env * 2] : 0xFFFFFFFFu, cm1 = cmask ? cmask[(size_t)env * 2 + 1] : 0xFFFFFFFFu;
    const unsigned um0 = umask ? umask[0] : 0xFFFFFFFFu, um1 = umask ? umask[1] : 0xFFFFFFFFu;
    for (int i = tid; i < 49 * 16; i += 256) {
        const int p = i >> 4;
        if (!((p < 32 ? um0 >> p : um1 >> (p - 32)) & 1u)) continue;
        const bool aff = ((p < 32 ? cm0 >> p : cm1 >> (p - 32)) & 1u) != 0;
        float4 v = aff ? reinterpret_cast<const float4 *>(z3sh + (size_t)env * 3136)[i] : reinterpret_cast<const float4 *>(z3bg)[i & 15];
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        reinterpret_cast<float4 *>(a3sh + (size_t)env * 3136)[i] = v;
    }
}

// Row order: by the item's set of live taps -- (rows of conv3's kernel that reach one of the agent's cells) x (columns), 3 + 3 bits,
// 0 for a pixel outside the agent's own support -- so that a 256-row tile multiplies exactly the taps its rows have (the order inside
// a key is whatever the LDS cursors hand out: every row is computed and stored on its own, so the results do not depend on it).
constexpr int PITEM_KEYS = 64;
struct PItemGeom {
    int oy, ox, H, Wc, loy, hiy, lox, hix;
    unsigned sm;
    __device__ __forceinline__ void load(int m, const unsigned *smask, const signed char *org, const uint8_t *pos, const int *cslot) {
        sm = smask ? smask[m] : 0x1FFFFFFu;
        oy = org[m] / 3;
        ox = org[m] - oy * 3;
        H = (pos[(size_t)m * 2] >> 2) >> 1;
        Wc = (pos[(size_t)m * 2 + 1] >> 2) >> 1;
        unsigned vy = 0, vx = 0;      // canonical cell rows / columns the agent has (conv2_cover is separable per axis)
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (cslot[(size_t)m * 9 + j] >= 0) { vy |= 1u << (j / 3); vx |= 1u << (j % 3); }
        loy = vy ? __ffs(vy) - 1 : 3; hiy = vy ? 31 - __clz(vy) : 0; lox = vx ? __ffs(vx) - 1 : 3; hix = vx ? 31 - __clz(vx) : 0;
    }
    // patch pixel q: the cell of tap (0,0) per axis and the key (ymask << 3 | xmask)
    __device__ __forceinline__ int key(int q, int &cy0, int &cx0) const {
        const int py = q / 5, px = q - py * 5;
        cy0 = H - (oy + py);
        cx0 = Wc - (ox + px);
        if (!((sm >> q) & 1u)) return 0;
        unsigned ym = 0, xm = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (cy0 - t >= loy && cy0 - t <= hiy) ym |= 1u << t;
            if (cx0 - t >= lox && cx0 - t <= hix) xm |= 1u << t;
        }
        return (ym && xm) ? (int)((ym << 3) | xm) : 0;
    }
};
// per workgroup of 256 samples: how many items of each key
__global__ __launch_bounds__(256) void pitem_count_kernel(const unsigned *__restrict__ wmask, const unsigned *__restrict__ smask, int n,
                                                          const signed char *__restrict__ org, const uint8_t *__restrict__ pos,
                                                          const int *__restrict__ cslot, int *__restrict__ cnt) {
    __shared__ int hist[PITEM_KEYS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid;
    if (tid < PITEM_KEYS) hist[tid] = 0;
    __syncthreads();
    const unsigned wm = m < n ? (wmask ? wmask[m] : 0x1FFFFFFu) : 0u;
    if (wm) {
        PItemGeom g;
        g.load(m, smask, org, pos, cslot);
        for (unsigned w = wm; w; w &= w - 1) {
            int cy0, cx0;
            atomicAdd(&hist[g.key(__ffs(w) - 1, cy0, cx0)], 1);
        }
    }
    __syncthreads();
    if (tid < PITEM_KEYS) cnt[(size_t)blockIdx.x * PITEM_KEYS + tid] = hist[tid];
}
// off[b][k] = first row of workgroup b's items of key k.  Order of the rows (round 5): SUPER-BLOCKS of PITEM_SB workgroups (1 024
// samples) in memory order, inside a super-block key-major (key 0 -- no tap, the row is all zeros -- last), inside a key the workgroups
// in order.  The gather reads a sample's nine cells (2.3 KB) once per live (pixel, tap) pair, 81 times where every tap is live: with
// the rows key-major over the whole CHUNK (round 4) a key's tiles sweep all 189 MB of cells, and the launch moved 1.95 GB through the
// L2s at 5.2 TB/s -- at the roof of what lies behind them -- with every agent in the interior.  A super-block's cells are 2.4 MB, and
// the launch keeps a contiguous range of row tiles on one XCD (gemm_rowk, XCD_ORDER = 2), so the re-reads of a super-block hit that
// XCD's 4 MB L2.  (Round 4 had tried super-blocks WITHOUT the XCD ranges, on the rim workload: nothing -- eight L2s each fetched
// every super-block.)  A tile that straddles two keys multiplies the union of their taps: ~50 such tiles per super-block of ~150.
// A wave per super-block (16 waves walk them): lane i holds key (i + 1) & 63 -- the key order -- and the super-block's PITEM_SB counts
// of that key, all requested together; totals by a wave sum, the super-blocks' exclusive scan by one shuffle scan, a key's base inside
// its super-block by a wave scan.  (The first form of this order, one THREAD per super-block walking its 256 counts twice, was a
// 64-step chain of cache round trips: 42 us at 4 096 envs where the key-major scan of round 4 took 8.)
constexpr int PITEM_SB = 4;
__global__ __launch_bounds__(1024) void pitem_scan_kernel(const int *__restrict__ cnt, int nb, int *__restrict__ off, int *__restrict__ rows_n) {
    __shared__ int R[256], wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, key = (lane + 1) & (PITEM_KEYS - 1);
    const int nsb = (nb + PITEM_SB - 1) / PITEM_SB;      // <= 256 (checked by the caller)
    if (tid < 256) R[tid] = 0;
    __syncthreads();
    for (int s = wave; s < nsb; s += 16) {
        int t = 0;
#pragma unroll
        for (int b = 0; b < PITEM_SB; ++b) {
            const int blk = s * PITEM_SB + b;
            t += blk < nb ? cnt[(size_t)blk * PITEM_KEYS + key] : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if (lane == 0) R[s] = t;
    }
    __syncthreads();
    if (tid < 256) {      // exclusive scan of the super-blocks' totals
        const int v = R[tid];
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        R[tid] = incl - v;      // (completed below, after the waves' totals are there)
    }
    __syncthreads();
    if (tid < 256) {
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wtot[w];
        R[tid] += base;
        if (tid == 0) *rows_n = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    }
    __syncthreads();
    for (int s = wave; s < nsb; s += 16) {
        int c[PITEM_SB], t = 0;
#pragma unroll
        for (int b = 0; b < PITEM_SB; ++b) {
            const int blk = s * PITEM_SB + b;
            c[b] = blk < nb ? cnt[(size_t)blk * PITEM_KEYS + key] : 0;
            t += c[b];
        }
        int incl = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        int run = R[s] + incl - t;
#pragma unroll
        for (int b = 0; b < PITEM_SB; ++b) {
            const int blk = s * PITEM_SB + b;
            if (blk < nb) off[(size_t)blk * PITEM_KEYS + key] = run;
            run += c[b];
        }
    }
}
// the items' rows: gather descriptor and live-tap mask of row off[b][key] + (the key's cursor in this workgroup)
__global__ __launch_bounds__(256) void pitem_place_kernel(const unsigned *__restrict__ wmask, const unsigned *__restrict__ smask, int n,
                                                          const signed char *__restrict__ org, const uint8_t *__restrict__ pos,
                                                          const int *__restrict__ cslot, const int *__restrict__ cinv,
                                                          const unsigned *__restrict__ cmask, const int *__restrict__ off, int4 *__restrict__ desc,
                                                          unsigned short *__restrict__ tapm) {
    __shared__ int cursor[PITEM_KEYS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid;
    if (tid < PITEM_KEYS) cursor[tid] = off[(size_t)blockIdx.x * PITEM_KEYS + tid];
    __syncthreads();
    const unsigned wm = m < n ? (wmask ? wmask[m] : 0x1FFFFFFu) : 0u;
    if (!wm) return;
    PItemGeom g;
    g.load(m, smask, org, pos, cslot);
    const int env = m / 10, crow = cinv[m];
    const unsigned cm0 = cmask ? cmask[(size_t)env * 2] : 0xFFFFFFFFu, cm1 = cmask ? cmask[(size_t)env * 2 + 1] : 0xFFFFFFFFu;
    for (unsigned w = wm; w; w &= w - 1) {
        const int q = __ffs(w) - 1;
        int cy0, cx0;
        const int key = g.key(q, cy0, cx0);
        const int r = atomicAdd(&cursor[key], 1);
        const int py = q / 5, px = q - py * 5, p = (g.oy + py) * 7 + g.ox + px;
        const bool inside = (g.sm >> q) & 1u;
        unsigned taps = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t)
            if (((key >> (3 + t / 3)) & 1) && ((key >> (t % 3)) & 1)) taps |= 1u << t;
        const bool aff = ((p < 32 ? cm0 >> p : cm1 >> (p - 32)) & 1u) != 0;
        desc[r] = make_int4((inside ? (1 << 30) : 0) | (aff ? (1 << 29) : 0) | (p << 23) | (m << 5) | q, crow * 576 + (cy0 * 3 + cx0) * 64,
                            key, 0);
        tapm[r] = (unsigned short)taps;
    }
}
// per 128-row tile: the union of its rows' live taps; the rows behind the live count of the last tile become dead descriptors
__global__ __launch_bounds__(128) void pitem_masks_kernel(int4 *__restrict__ desc, const unsigned short *__restrict__ tapm,
                                                          const int *__restrict__ rows_n, unsigned short *__restrict__ tmask) {
    __shared__ unsigned part[2];
    const int live = *rows_n, r = blockIdx.x * 128 + threadIdx.x;
    if (blockIdx.x * 128 >= live) return;
    unsigned v = 0;
    if (r < live) v = tapm[r];
    else desc[r] = make_int4(-1, 0, 0, 0);      // no live tap, nothing stored
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tmask[blockIdx.x] = (unsigned short)(part[0] | part[1]);
}

// where the conv3 patch gather's operands and lists live: the a2 buffer has no other use in shared-trunk mode -- canonical cells
// (ctiles * 256 rows, written by EpiConv2Corr), then the items' rows
struct PItemBufs { float *d2c; int4 *desc; unsigned short *tapm, *tmask9; int *icnt, *ioff, *irows; };
static PItemBufs pitem_bufs(grl_net *net) {
    const size_t c = net->chunk, nbmax = (c + 255) / 256;
    PItemBufs b;
    b.d2c = net->a2;
    b.desc = reinterpret_cast<int4 *>(net->a2 + (size_t)net->ctiles * 256 * 576);
    b.tapm = reinterpret_cast<unsigned short *>(b.desc + c * 25 + 256);
    b.tmask9 = b.tapm + c * 25 + 256;
    b.icnt = reinterpret_cast<int *>(b.tmask9 + ((c * 25 + 127) / 128 + 8) / 2 * 2 + 2);
    b.ioff = b.icnt + nbmax * PITEM_KEYS;
    b.irows = b.ioff + nbmax * PITEM_KEYS;
    return b;
}
static bool pitem_gather_on(const grl_net *net) { return net->expand3_gather && net->expand2_gemm && net->chunk <= (1u << 17); }      // a row's code word holds 17 bits of sample index
// the item sort of the gather on the handle's current stream: needs the patch sort's wmask / smask / org, the class sort's cinv, cslot,
// and (list form) the trunk's cmask -- nothing the forward pass COMPUTES, so it may run on the lane's index side stream
static int pitem_index(grl_net *net, int n, const uint8_t *pos) {
    hipStream_t st = net->h->stream;
    const PItemBufs b = pitem_bufs(net);
    const bool trunk3f = net->trunk_skip && net->expand2_gemm;
    const unsigned *wm = net->patch_skip ? net->wmask : nullptr, *smk = net->patch_skip ? net->smask : nullptr;
    const int nb = (n + 255) / 256;
    if ((nb + PITEM_SB - 1) / PITEM_SB > 256) return paac_fail(net, GRL_E_INVALID, "pitem_index: chunk too large for the item scan");
    hipLaunchKernelGGL(pitem_count_kernel, dim3(nb), dim3(256), 0, st, wm, smk, n, (const signed char *)net->org, pos, (const int *)net->cslot, b.icnt);
    hipLaunchKernelGGL(pitem_scan_kernel, dim3(1), dim3(1024), 0, st, (const int *)b.icnt, nb, b.ioff, b.irows);
    hipLaunchKernelGGL(pitem_place_kernel, dim3(nb), dim3(256), 0, st, wm, smk, n, (const signed char *)net->org, pos, (const int *)net->cslot,
                       (const int *)net->cinv, trunk3f ? (const unsigned *)net->tcmask : (const unsigned *)nullptr, (const int *)b.ioff, b.desc, b.tapm);
    // 128-row tiles: the loop is bound by the latency of the gathers, and twice the workgroups per CU keep twice the loads in flight
    // (256-row tiles: 153 -> 122 us per chunk on the bench workload, 470 -> 392 us with every agent in the interior)
    const int tiles = (n * 25 + 127) / 128;
    hipLaunchKernelGGL(pitem_masks_kernel, dim3(tiles), dim3(128), 0, st, b.desc, (const unsigned short *)b.tapm, (const int *)b.irows, b.tmask9);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// conv3 + dense1 forward of one chunk on the shared tensors (a2sh, d2s, ulist from forward_conv12_shared)
static int forward_conv3_dense1_shared(grl_net *net, int nenv, const uint8_t *pos) {
    hipStream_t st = net->h->stream;
    const float *P = net->params, *PT = net->paramsT;
    const int n = nenv * 10;
    const bool trunk3f = net->trunk_skip && net->expand2_gemm;
    if (trunk3f) {      // the conv3 outputs whose window holds an affected conv2 output; the rest is the background row (expand_conv3_patch substitutes it)
        GatherConv3Rows g{net->a2sh, net->tc3list, net->trows_n + 2, net->tbgimg3, nenv * 49, 1};
        EpiBiasDualRows e{net->z3sh, nullptr, 64, P + ConvOffsets::c3b, net->tc3list, net->trows_n + 2, nullptr, nullptr};
        net->prof_tag_cur = PT_ENV_FWD;
        {
            GemmTimer t(net, 2.0 * trunk_live(net, 2, (double)nenv * 49) * 576 * 64);
            launch_rowk<256, 64, kW256M, kW256N, GatherConv3Rows, EpiBiasDualRows>(net, dim3(1, (nenv * 49 + 255) / 256), st, g, PT + ConvOffsets::c3w, 576, 64, e);
        }
    } else {
        GatherConv3 g{net->a2sh, nenv * 49};
        EpiBiasAct e{net->z3sh, 64, P + ConvOffsets::c3b, ACT_NONE};
        net->prof_tag_cur = PT_ENV_FWD;
        GemmTimer t(net, 2.0 * nenv * 49 * 576 * 64);
        launch_rowk<256, 64, kW256M, kW256N, GatherConv3, EpiBiasAct>(net, dim3(1, (nenv * 49 + 255) / 256), st, g, PT + ConvOffsets::c3w, 576, 64, e);
    }
    if (pitem_gather_on(net)) {
        // the agents' corrections of conv3 gathered at their patch pixels (SlotsToPatch, net_gemm.h): no slot-product tensor, no expansion kernel
        const PItemBufs pb = pitem_bufs(net);
        float *d2c = pb.d2c;
        int4 *desc = pb.desc;
        unsigned short *tmask9 = pb.tmask9;
        int *irows = pb.irows;
        hipLaunchKernelGGL(a3sh_relu_kernel, dim3(nenv), dim3(256), 0, st, (const float *)net->z3sh,
                           trunk3f ? (const unsigned *)net->tcmask : (const unsigned *)nullptr, (const float *)net->tbgz3,
                           trunk3f ? (const unsigned *)net->tumask : (const unsigned *)nullptr, net->a3sh);
        if (net->pitem_on_side) net->pitem_on_side = 0;      // this pass's item lists came from the side stream (forward_conv12_shared)
        else if (int rc = pitem_index(net, n, pos)) return rc;
        const int maxrows = n * 25, tiles = (maxrows + 127) / 128;
        double live_pairs = (double)maxrows * 9;      // FLOP count of the profiling pass: rows x live taps of their tile
        if (net->prof_on) {
            int nlive = 0;
            PAAC_HIP(net, hipStreamSynchronize(st));
            PAAC_HIP(net, hipMemcpy(&nlive, irows, sizeof(int), hipMemcpyDeviceToHost));
            const int nt = (nlive + 127) / 128;
            std::vector<unsigned short> tm(nt > 0 ? nt : 1);
            if (nt > 0) PAAC_HIP(net, hipMemcpy(tm.data(), tmask9, (size_t)nt * 2, hipMemcpyDeviceToHost));
            live_pairs = 0;
            for (int t = 0; t < nt; ++t) live_pairs += 128.0 * __builtin_popcount(tm[t] & 0x1FFu);
        }
        SlotsToPatch g{d2c, desc, maxrows, irows, tmask9};
        EpiPatchExpand e{desc, net->z3sh, (const float *)net->tbgz3, net->d3, net->m3};
        net->prof_tag_cur = PT_SLOT_FWD;
        GemmTimer t(net, 2.0 * live_pairs * 64 * 64);
        // a contiguous range of the (super-block-major) row tiles per XCD: XCD_ORDER = 2 (8 more workgroups than tiles: the ranges' round-up)
        if (net->slots_xcd)
            launch_rowk<128, 64, 4, 1, SlotsToPatch, EpiPatchExpand, 2, true, 1, true>(net, dim3(1, tiles + 8), st, g, PT + ConvOffsets::c3w, 576, 64, e);
        else
            launch_rowk<128, 64, 4, 1, SlotsToPatch, EpiPatchExpand, 1, true, 1, true>(net, dim3(1, tiles), st, g, PT + ConvOffsets::c3w, 576, 64, e);
    } else {
    {   // prod[(agent, slot)][(tap, co)] = (a2_a - a2sh)[u] . W3[tap][:, co]
        // compact slot rows in tap-class order: tiles past the live count exit, column tiles of taps no row of the tile has live are skipped
        SlotRowsP g{net->d2s, net->sperm, n * 9, 64, 64, net->sbase + n, net->patch_skip ? net->stmask : nullptr};
        EpiPermStore e{net->a2, net->sperm, 576};
        net->prof_tag_cur = PT_SLOT_FWD;
        GemmTimer t(net, 2.0 * slot_rows_for_flops(net, n) * 64 * 576 * net->sfrac);
        launch_rowk<256, 64, kW256M, kW256N, SlotRowsP, EpiPermStore>(net, dim3(576 / 64, (n * 9 + 255) / 256), st, g, net->w3f, 64, 576, e);
    }
    maybe_evict(net);
    hipLaunchKernelGGL(expand_conv3_patch_kernel, dim3(nenv), dim3(256), 0, st, net->z3sh, net->a2, net->ulist, net->sbase, net->org,
                       net->patch_skip ? net->smask : nullptr, net->patch_skip ? net->wmask : nullptr, net->a3sh, net->d3, net->m3,
                       trunk3f ? (const unsigned *)net->tcmask : (const unsigned *)nullptr, (const float *)net->tbgz3,
                       trunk3f ? (const unsigned *)net->tumask : (const unsigned *)nullptr);
    }
    if (trunk3f) {   // per-env part of dense1 over the pixels of the chunk's union mask; the background's share of the rest rides in the bias
        static_assert(3136 <= DenseRowsKU::kMaxK, "the union mask's 64 bits cover K");
        DenseRowsKU g{{net->a3sh, nenv, 3136, 3136}, net->tumask};
        EpiBiasAct e{net->ysh, 512, net->tubias, ACT_NONE};
        net->prof_tag_cur = PT_ENV_FWD;
        GemmTimer t(net, 2.0 * nenv * 64.0 * trunk_union_pixels(net) * 512);
        launch_rowk<128, 64, 4, 1, DenseRowsKU, EpiBiasAct, true, true, 2>(net, dim3(512 / 64, (nenv + 127) / 128), st, g, PT + ConvOffsets::d1w, 3136, 512, e);
    } else {   // per-env part of dense1 (bias included)
        DenseRows g{net->a3sh, nenv, 3136, 3136};
        EpiBiasAct e{net->ysh, 512, P + ConvOffsets::d1b, ACT_NONE};
        net->prof_tag_cur = PT_ENV_FWD;
        GemmTimer t(net, 2.0 * nenv * 3136 * 512);
        // 128 x 64 tiles: 4 096 rows x 512 columns give 256 workgroups (one per CU) instead of 128
        launch_rowk<128, 64, 4, 1, DenseRows, EpiBiasAct>(net, dim3(512 / 64, (nenv + 127) / 128), st, g, PT + ConvOffsets::d1w, 3136, 512, e);
    }
    {   // per-agent patch part: d1 = relu(ysh[env] + d3 . W[patch rows])
        static_assert(1600 <= PatchRows::kMaxK0, "the support word's 32 bits cover the patch");
        PatchRows g{net->d3, net->perm, net->tilegroup, net->ptiles * 256, 1600, 1600, 0, nullptr, nullptr, net->patch_skip ? net->tmask : nullptr, nullptr};
        EpiPatchFwd e{net->d1, net->ysh, net->perm, 512};
        net->prof_tag_cur = PT_PATCH_FWD;
        GemmTimer t(net, 2.0 * n * 1600 * 512 * net->pfrac[0]);
        launch_rowk<128, 128, kW128M, kW128N, PatchRows, EpiPatchFwd, true, false, 2>(net, dim3(512 / 128, net->ptiles * 2), st, g, PT + ConvOffsets::d1w, 3136, 512, e);
    }
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// ------------------------------------------------------------------------------------------ backward pieces
// conv3-output gradients of the dense1 split.  On entry gsh3[e] = (sum_a gd1_a) . W^T over all 3136 inputs (no mask) and
// g3p[m] = gd1_m . W[patch rows]^T (no mask).  The env's summed dz3 is
//     DZ3[e][r] = relu'(a3sh[r]) . gsh3[e][r] + sum over agents whose patch holds r of (relu'(a3_a[r]) - relu'(a3sh[r])) . g3p_a[r]
// and the per-agent dz3 inside the patch, dz3p[m] = relu'(a3_a) . g3p[m], feeds the slot-gather conv3 corrections.
// One workgroup per env (strided); agents are folded in order (their patches overlap).
// Round 4, after agent_dz2_kernel (net_shared.inc): a lane owns FOUR consecutive channels of a pixel (16 lanes per pixel: 16-byte loads
// and stores, a quarter of the index arithmetic and LDS updates), the shared mask is kept as one nibble per lane instead of a second
// 12.5 KB image, and an agent's operands are fetched while the agent before it is folded (the fold is fully unrolled: the prefetched
// values are new registers, not loop-carried copies that would wait for their loads at the end of the same round).
__global__ __launch_bounds__(256, 6) void agent_dz3_kernel(const float *__restrict__ gsh3, const float *__restrict__ g3p,
                                                        const float *__restrict__ a3sh, const unsigned long long *__restrict__ m3,
                                                        const signed char *__restrict__ org, const unsigned *__restrict__ smask, int nenv,
                                                        float *__restrict__ dz3sh, float *__restrict__ dz3p, float *__restrict__ bsum,
                                                        const unsigned *__restrict__ cmask, float *__restrict__ bgsum,
                                                        const float *__restrict__ a3bg, const unsigned *__restrict__ umask) {
    __shared__ __attribute__((aligned(16))) float acc[49 * 64];
    __shared__ unsigned cm[2];
    // umask: the chunk's union of the cmasks.  Outside it gsh3 was not computed (DenseRowsNU) and nothing here is per env: the sums
    // those pixels contribute come from trunk_upix / trunk_uadd in closed form
    const unsigned um0 = umask ? umask[0] : 0xFFFFFFFFu, um1 = umask ? umask[1] : 0xFFFFFFFFu;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cs = zero4;      // channels 4 (tid & 15) .. + 3 of the dz3sh this workgroup writes, summed over pixels and envs (conv3's bias gradient)
    float4 cb = zero4;      // ... and over the pixels outside the env's affected set (cmask: the rank-1 term of conv3's weight gradient)
    __shared__ unsigned char mskn[49 * 16];      // sign nibble of the env's a3sh per (pixel, lane of 4 channels): the shared mask
    __shared__ int og[10], pcnt[10];
    __shared__ unsigned char plist[10][28];      // the pixels of each agent's support, ascending
    const int tid = threadIdx.x, l16 = tid & 15, c4 = l16 * 4;
    float4 bg4 = zero4;
    if (a3bg) bg4 = *reinterpret_cast<const float4 *>(a3bg + c4);
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        if (tid >= 64 && tid < 66) cm[tid - 64] = cmask ? cmask[(size_t)env * 2 + tid - 64] : 0xFFFFFFFFu;
        if (tid < 10) {
            og[tid] = org[(size_t)env * 10 + tid];
            // Outside the agent's support (smask, net_patch.inc) its a3 IS the shared one: same mask, no correction, and nobody reads
            // dz3p there (the slot gathers stay inside the support) -- so those pixels are neither read nor written, and the data
            // gradient GEMM does not store them (PatchRows::n_ok).  smask == nullptr: the whole 5x5 patch, as before.
            const unsigned sm = smask ? smask[(size_t)env * 10 + tid] : 0x1FFFFFFu;
            int c = 0;
            for (int q = 0; q < 25; ++q)
                if ((sm >> q) & 1u) plist[tid][c++] = (unsigned char)q;
            pcnt[tid] = c;
        }
        __syncthreads();      // cm, og, plist
        {   // the env's image: shared mask and the shared-mask part of DZ3, four passes of 16-byte loads in flight together
            float4 sv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = tid + 256 * k, p = i >> 4;      // float4 index, pixel
                sv[k] = bg4;
                gv[k] = zero4;
                // outside the union nothing is per env; outside the env's affected set a3sh IS the background row (a3bg != nullptr: list
                // form): no read.  (The mask stays the background's there: an agent outside the box has no slots but a one-pixel
                // support, which may lie out here; its correction is (own mask - shared mask) . g = 0 only against the right shared mask)
                if (i < 49 * 16 && ((p < 32 ? um0 >> p : um1 >> (p - 32)) & 1u)) {
                    if (!a3bg || ((cm[p >> 5] >> (p & 31)) & 1u)) sv[k] = reinterpret_cast<const float4 *>(a3sh + (size_t)env * 3136)[i];
                    gv[k] = reinterpret_cast<const float4 *>(gsh3 + (size_t)env * 3136)[i];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = tid + 256 * k;
                if (i < 49 * 16) {
                    const float4 s = sv[k], g = gv[k];
                    mskn[i] = (unsigned char)((s.x > 0.f ? 1 : 0) | (s.y > 0.f ? 2 : 0) | (s.z > 0.f ? 4 : 0) | (s.w > 0.f ? 8 : 0));
                    reinterpret_cast<float4 *>(acc)[i] = make_float4(s.x > 0.f ? g.x : 0.f, s.y > 0.f ? g.y : 0.f, s.z > 0.f ? g.z : 0.f, s.w > 0.f ? g.w : 0.f);
                }
            }
        }
        // items (agent, pass): pass r covers the support's lanes tid + 256 r (pixel of the list = lane >> 4); item 0's operands now
        int qn = -1;
        float4 gn = zero4;
        unsigned bn = 0;
#define GRL_DZ3_FETCH(a_, r_)                                                                                             \
        {                                                                                                                  \
            const int e_ = tid + 256 * (r_);                                                                               \
            qn = e_ < pcnt[a_] * 16 ? (int)plist[a_][e_ >> 4] : -1;                                                        \
            if (qn >= 0) {                                                                                                 \
                const size_t m_ = (size_t)env * 10 + (a_);                                                                \
                gn = *reinterpret_cast<const float4 *>(g3p + m_ * 1600 + qn * 64 + c4);                                    \
                bn = reinterpret_cast<const unsigned *>(m3)[(m_ * 25 + qn) * 2 + (c4 >> 5)];                               \
            }                                                                                                              \
        }
        GRL_DZ3_FETCH(0, 0)
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 10; ++a) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int q = qn;
                const float4 g = gn;
                const unsigned bits = (bn >> (c4 & 31)) & 0xFu;
                if (r == 0) GRL_DZ3_FETCH(a, 1)
                else if (a < 9) GRL_DZ3_FETCH(a + 1, 0)
                if (q >= 0) {
                    const int oy = og[a] / 3, ox = og[a] - oy * 3, py = q / 5, px = q - py * 5, i = ((oy + py) * 7 + ox + px) * 16 + l16;
                    const float4 ga = make_float4((bits & 1u) ? g.x : 0.f, (bits & 2u) ? g.y : 0.f, (bits & 4u) ? g.z : 0.f, (bits & 8u) ? g.w : 0.f);
                    const unsigned sh = mskn[i];
                    float4 c = reinterpret_cast<float4 *>(acc)[i];
                    c.x += ga.x - ((sh & 1u) ? g.x : 0.f);
                    c.y += ga.y - ((sh & 2u) ? g.y : 0.f);
                    c.z += ga.z - ((sh & 4u) ? g.z : 0.f);
                    c.w += ga.w - ((sh & 8u) ? g.w : 0.f);
                    reinterpret_cast<float4 *>(acc)[i] = c;
                    *reinterpret_cast<float4 *>(dz3p + ((size_t)env * 10 + a) * 1600 + q * 64 + c4) = ga;
                }
            }
            __syncthreads();
        }
#undef GRL_DZ3_FETCH
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + 256 * k, p = i >> 4;
            if (i < 49 * 16) {
                const bool aff = (cm[p >> 5] >> (p & 31)) & 1u;
                const float4 v = reinterpret_cast<const float4 *>(acc)[i];
                if (aff || !a3bg) reinterpret_cast<float4 *>(dz3sh + (size_t)env * 3136)[i] = v;
                cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w;
                if (!aff) { cb.x += v.x; cb.y += v.y; cb.z += v.z; cb.w += v.w; }
            }
        }
    }
    __syncthreads();      // fold the sixteen lanes per channel quad in lane-group order (acc is free now)
    reinterpret_cast<float4 *>(acc)[tid] = cs;
    reinterpret_cast<float4 *>(acc)[256 + tid] = cb;
    __syncthreads();
    if (tid < 128) {
        const int c = tid & 63, base = tid < 64 ? 0 : 1024;
        float t = 0.f;
#pragma unroll
        for (int gq = 0; gq < 16; ++gq) t += acc[base + (gq * 16 + (c >> 2)) * 4 + (c & 3)];
        if (tid < 64) bsum[(size_t)blockIdx.x * 64 + c] = t;
        else if (bgsum) bgsum[(size_t)blockIdx.x * 64 + c] = t;
    }
}

// (patch_dw_reduce_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)
