// Included by net_conv.hip: loss + backward + optimiser of ConvSingleAgentPolicyNetwork and the
// device-resident PAAC rollout.  Reference: fed_gym/agents/paac/policy_v_network.py:45-66 (loss),
// fed_gym/agents/paac/actor_learner.py:31-68 (Adam, clip_by_global_norm),
// fed_gym/agents/paac/paac.py:302-387 (GridPAACLearner.train inner loop).
//
// Backward per chunk of n agent-samples (activations recomputed by forward_chunk):
//   heads_backward           loss terms, d/dz of mu/sigma/value heads, grads wrt p1 and v2
//   gemm_rowk                data gradients of the dense stack (dY * W^T, ReLU mask fused)
//   gemm_rowk + GatherT3/T2  data gradients of conv3 / conv2 as gather-form transposed convolutions
//   gemm_tn                  weight gradients (A^T dY), split over rows into slabs, reduced in fixed order
//   conv1_wgrad              sparse weight gradient of conv1 from the compact observation
// All partial sums are combined in a fixed order, so a gradient is bitwise reproducible run to run
// (conv1's LDS accumulation is float64, its order-dependence is below float32 resolution).

#include "net_slab_plan.h"

namespace grl {

static inline double host_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the chunk's queued reductions (net_reduce.inc) and the bump allocation of their source regions
static int rq_flush(grl_net *net) {
    const int nj = (int)net->rq.size();
    if (!nj) { net->slab_used = 0; net->slabb_used = 0; return GRL_OK; }
    std::vector<int> phase(nj, 0);
    int maxph = 0;
    for (int k = 0; k < nj; ++k) {
        for (int i = 0; i < k; ++i) phase[k] += net->rq_dst[i] == net->rq_dst[k];
        maxph = std::max(maxph, phase[k]);
    }
    for (int ph = 0; ph <= maxph; ++ph) {
        int k = 0;
        while (k < nj) {
            RBatch B;
            B.njobs = 0;
            int blocks = 0;
            for (; k < nj && B.njobs < kRJobs; ++k) {
                if (phase[k] != ph) continue;
                B.bstart[B.njobs] = blocks;
                B.j[B.njobs++] = net->rq[k];
                blocks += net->rq[k].blocks;
            }
            if (!B.njobs) break;
            B.bstart[B.njobs] = blocks;
            hipLaunchKernelGGL(reduce_batch_kernel, dim3(blocks), dim3(256), 0, net->h->stream, B);
        }
    }
    net->rq.clear(); net->rq_dst.clear();
    net->slab_used = 0; net->slabb_used = 0;
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}
// a few independent jobs NOW, as one launch (their results feed kernels of the same chunk)
static void rb_launch(grl_net *net, const RJob *jobs, int n) {
    RBatch B;
    B.njobs = n;
    int blocks = 0;
    for (int k = 0; k < n; ++k) { B.bstart[k] = blocks; B.j[k] = jobs[k]; blocks += jobs[k].blocks; }
    B.bstart[n] = blocks;
    hipLaunchKernelGGL(reduce_batch_kernel, dim3(blocks), dim3(256), 0, net->h->stream, B);
}
static void rq_push(grl_net *net, int dst, const RJob &j) {
    net->rq.push_back(j);
    net->rq_dst.push_back(dst);
}
// `count` floats of the split-M slab buffer that stay untouched until the queue is flushed (a full buffer flushes it first);
// nullptr when the request alone is larger than the buffer
static float *slab_take(grl_net *net, size_t count) {
    count = (count + 63) & ~(size_t)63;
    if (count > net->slab_floats) return nullptr;
    if (net->slab_used + count > net->slab_floats && rq_flush(net) != GRL_OK) return nullptr;
    float *p = net->slab + net->slab_used;
    net->slab_used += count;
    return p;
}
static size_t slab_left(grl_net *net) { return net->slab_floats; }      // what ONE request may ask for (slab_take flushes to make room)
static float *slabb_take(grl_net *net, size_t count) {
    count = (count + 63) & ~(size_t)63;
    if (count > net->slabb_floats) return nullptr;
    if (net->slabb_used + count > net->slabb_floats && rq_flush(net) != GRL_OK) return nullptr;
    float *p = net->slabb + net->slabb_used;
    net->slabb_used += count;
    return p;
}

// the slabs of a split-M launch: sized by slab_plan (net_slab_plan.h), taken from the slab buffer; `what` is the call site's message
// (nullptr with the message set: the caller returns GRL_E_INVALID)
static float *slab_plan_take(grl_net *net, int wg_target, int tiles, int min_chunks, int rows, size_t floats_per_chunk, const char *what,
                             int *chunks, int *mc = nullptr) {
    const SlabPlan pl = slab_plan(wg_target, tiles, min_chunks, rows, floats_per_chunk, slab_left(net));
    float *slab = pl.chunks < 1 ? nullptr : slab_take(net, (size_t)pl.chunks * floats_per_chunk);
    if (!slab) paac_fail(net, GRL_E_INVALID, what);
    *chunks = pl.chunks;
    if (mc) *mc = pl.mc;
    return slab;
}

constexpr size_t kSlab64Doubles = (size_t)2048 * 4096;      // float64 partials of the conv1 weight gradient: <= 2048 workgroups x 4096 (or 512 x 6144)
constexpr float LOG_2PI_F = 1.8378770664093453f;

// ------------------------------------------------------------------------------------------ heads backward
// slab[chunk] = [muw 512xA | mub A | sgw 512xA | sgb A | v3w 256 | v3b 1 | policy / critic loss-term sums]  (flat-vector order)
__host__ __device__ inline int heads_slab(int A) { return 1024 * A + 2 * A + 256 + 1 + 2; }
template <int A>
__global__ __launch_bounds__(256) void heads_backward_kernel(const float *__restrict__ p1, const float *__restrict__ v2,
                                                             const float *__restrict__ mu, const float *__restrict__ sigma,
                                                             const float *__restrict__ vs, const float *__restrict__ actions,
                                                             const float *__restrict__ adv, const float *__restrict__ y,
                                                             const float *__restrict__ params, HeadOff ho, int n, float scale, float beta,
                                                             float inv_total, const float *__restrict__ lscale, float *__restrict__ gp1,
                                                             float *__restrict__ gv2, float *__restrict__ dzh, double *__restrict__ stats64,
                                                             float *__restrict__ slab) {
    // kHeadRows rows per wave, a lane owns columns 4 lane .. + 3 of each 256-wide block: the head weights of those columns sit in
    // registers and the 3 kHeadRows 16-byte activation loads are in flight together (one row per wave with 4-byte loads waited 86 %
    // of its wave cycles, round 2).  Every element is the same sum in the same order as before.
    // The HEAD WEIGHT GRADIENTS ride along (round 3): the activations a lane holds are exactly the rows of muw / sgw / v3w it owns,
    // so x . dz is accumulated in registers over the row blocks a workgroup walks (blocks blockIdx.x, + gridDim.x, ...), the four
    // waves are folded in wave order through LDS, and the workgroup writes ONE slab row in the layout of heads_slab() -- the
    // separate weight-gradient kernel read p1 and v2 (252 MB per chunk) a second time.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *muw = params + ho.muw, *sgw = params + ho.sgw, *v3w = params + ho.v3w;
    float am[8][A], as_[8][A], av[4] = {0.f, 0.f, 0.f, 0.f}, ab[2 * A + 3];
    float bg1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bg2[4] = {0.f, 0.f, 0.f, 0.f};      // column sums of what is stored to gp1 / gv2: the bias gradients of pol1 and v2
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int a = 0; a < A; ++a) { am[j][a] = 0.f; as_[j][a] = 0.f; }
#pragma unroll
    for (int i = 0; i < 2 * A + 3; ++i) ab[i] = 0.f;
    float wm[8][A], ws[8][A];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = (j >> 2) * 256 + 4 * lane + (j & 3);
#pragma unroll
        for (int a = 0; a < A; ++a) { wm[j][a] = muw[k * A + a]; ws[j][a] = sgw[k * A + a]; }
    }
    const float wv[4] = {v3w[4 * lane], v3w[4 * lane + 1], v3w[4 * lane + 2], v3w[4 * lane + 3]};      // 8-byte aligned only for an odd A
    const float ls = lscale[0];      // every gradient of the pass carries this power of two (exact), removed by unscale_grads_kernel at the end
    for (int row0 = (blockIdx.x * 4 + wave) * kHeadRows; row0 < n; row0 += gridDim.x * 4 * kHeadRows) {
    float4 x0[kHeadRows], x1[kHeadRows], xv[kHeadRows];
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        const size_t row = (size_t)min(row0 + r, n - 1);      // clamped: the tail rows are loaded twice and not stored
        x0[r] = reinterpret_cast<const float4 *>(p1 + row * 512)[lane];
        x1[r] = reinterpret_cast<const float4 *>(p1 + row * 512 + 256)[lane];
        xv[r] = reinterpret_cast<const float4 *>(v2 + row * 256)[lane];
    }
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        if (row0 + r >= n) break;
        const int row = row0 + r;
        const float Adv = adv[row], v = vs[row], tgt = y[row];
        // Normal(mu, sigma).log_prob / entropy summed over the action dimensions (policy_v_network.py:45-53)
        const float dlogp = -Adv * inv_total * ls, dent = -beta * inv_total * ls;
        float zm[A], zs[A], logp = 0.f, ent = 0.f;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float m = mu[(size_t)row * A + a], s = sigma[(size_t)row * A + a], d = actions[(size_t)row * A + a] - m;
            const float lp = -0.5f * (d / s) * (d / s) - logf(s) - 0.5f * LOG_2PI_F, en = 0.5f + 0.5f * LOG_2PI_F + logf(s);
            logp = a == 0 ? lp : logp + lp;
            ent = a == 0 ? en : ent + en;
            const float dmu = dlogp * d / (s * s);
            const float dsg = dlogp * (d * d / (s * s * s) - 1.0f / s) + dent / s;
            zm[a] = dmu * (1.0f - m * m);          // tanh'
            zs[a] = dsg * s * (1.0f - s);          // sigmoid'
        }
        const float dvs = 0.5f * (v - tgt) / scale * inv_total * ls;      // d mean(0.25*(vs-y)^2/scale)
        // vs = -scale*softplus(z): dvs/dz = -scale*sigmoid(z), sigmoid(z) = 1 - exp(-softplus(z)) = -expm1(vs/scale)
        const float zv = dvs * (-scale) * (-expm1f(v / scale));
        if (lane == 0) {
            float *o = dzh + (size_t)row * ho.dz;
#pragma unroll
            for (int a = 0; a < A; ++a) { o[a] = zm[a]; o[A + a] = zs[a]; }
            o[2 * A] = zv;
            // loss terms of this row, summed later by heads_wgrad_kernel in a fixed order (no atomics)
            o[2 * A + 1] = -(logp * Adv + beta * ent);
            o[2 * A + 2] = 0.25f * (v - tgt) * (v - tgt) / scale;
        }
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = zm[0] * wm[j][0];
#pragma unroll
            for (int a = 1; a < A; ++a) t += zm[a] * wm[j][a];
#pragma unroll
            for (int a = 0; a < A; ++a) t += zs[a] * ws[j][a];
            // Keeps the eight sums scalar.  Left alone, the SLP vectorizer pairs neighbouring j's into v_pk_mul_f32 / v_pk_add_f32 with
            // op_sel half swaps, and that sequence was NOT reproducible on the MI355X: with two or more lanes (streams) busy, lanes
            // 48..63 of the low result (column 4 lane + 1 of the first block) changed in the last bits from pass to pass, while one
            // stream, or this barrier, gives bit-identical gradients (tools/diag_resident.py, round 3).
            asm volatile("" : "+v"(t));
            g[j] = t;
        }
        const float4 a0 = x0[r], a1 = x1[r], av_ = xv[r];
        {   // weight / bias gradients and the loss terms of this row
            const float xs[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int a = 0; a < A; ++a) { am[j][a] += xs[j] * zm[a]; as_[j][a] += xs[j] * zs[a]; }
            av[0] += av_.x * zv; av[1] += av_.y * zv; av[2] += av_.z * zv; av[3] += av_.w * zv;
#pragma unroll
            for (int a = 0; a < A; ++a) { ab[a] += zm[a]; ab[A + a] += zs[a]; }
            ab[2 * A] += zv;
            ab[2 * A + 1] += -(logp * Adv + beta * ent);
            ab[2 * A + 2] += 0.25f * (v - tgt) * (v - tgt) / scale;
        }
        const float4 o0 = make_float4(a0.x > 0.f ? g[0] : 0.f, a0.y > 0.f ? g[1] : 0.f, a0.z > 0.f ? g[2] : 0.f, a0.w > 0.f ? g[3] : 0.f);
        const float4 o1 = make_float4(a1.x > 0.f ? g[4] : 0.f, a1.y > 0.f ? g[5] : 0.f, a1.z > 0.f ? g[6] : 0.f, a1.w > 0.f ? g[7] : 0.f);
        const float4 ov = make_float4(av_.x > 0.f ? zv * wv[0] : 0.f, av_.y > 0.f ? zv * wv[1] : 0.f, av_.z > 0.f ? zv * wv[2] : 0.f, av_.w > 0.f ? zv * wv[3] : 0.f);
        reinterpret_cast<float4 *>(gp1 + (size_t)row * 512)[lane] = o0;
        reinterpret_cast<float4 *>(gp1 + (size_t)row * 512 + 256)[lane] = o1;
        reinterpret_cast<float4 *>(gv2 + (size_t)row * 256)[lane] = ov;
        bg1[0] += o0.x; bg1[1] += o0.y; bg1[2] += o0.z; bg1[3] += o0.w; bg1[4] += o1.x; bg1[5] += o1.y; bg1[6] += o1.z; bg1[7] += o1.w;
        bg2[0] += ov.x; bg2[1] += ov.y; bg2[2] += ov.z; bg2[3] += ov.w;
    }
    }
    // fold the four waves in wave order through ONE [value][lane] image: ((w0 + w1) + w2) + w3
    constexpr int NV = 16 * A + 16;      // muw, sgw rows (8 A each), v3w (4), pol1 bias (8), v2 bias (4) of this lane's columns
    __shared__ float red[NV][64];
    __shared__ float redb[2 * A + 3];
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    red[j * A + a][lane] = (w ? red[j * A + a][lane] : 0.f) + am[j][a];
                    red[8 * A + j * A + a][lane] = (w ? red[8 * A + j * A + a][lane] : 0.f) + as_[j][a];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) red[16 * A + i][lane] = (w ? red[16 * A + i][lane] : 0.f) + av[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) red[16 * A + 4 + j][lane] = (w ? red[16 * A + 4 + j][lane] : 0.f) + bg1[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) red[16 * A + 12 + i][lane] = (w ? red[16 * A + 12 + i][lane] : 0.f) + bg2[i];
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 2 * A + 3; ++i) redb[i] = (w ? redb[i] : 0.f) + ab[i];
        }
        __syncthreads();
    }
    constexpr int MUB = 512 * A, SG = 512 * A + A, SGB = 1024 * A + A, V3 = 1024 * A + 2 * A, HS = 1024 * A + 2 * A + 256 + 1 + 2;
    float *o = slab + (size_t)blockIdx.x * (HS + 768);      // a slab row = heads_slab(A) values, then pol1's bias row (512) and v2's (256)
    for (int e = threadIdx.x; e < NV * 64; e += 256) {
        const int vi = e >> 6, l = e & 63;
        const float t = red[vi][l];
        if (vi < 16 * A) {
            const int sg = vi >= 8 * A, q = vi - sg * 8 * A, j = q / A, a = q - j * A, k = (j >> 2) * 256 + 4 * l + (j & 3);
            o[(sg ? SG : 0) + k * A + a] = t;
        } else if (vi < 16 * A + 4) {
            o[V3 + 4 * l + (vi - 16 * A)] = t;
        } else if (vi < 16 * A + 12) {
            const int j = vi - (16 * A + 4);
            o[HS + (j >> 2) * 256 + 4 * l + (j & 3)] = t;
        } else {
            o[HS + 512 + 4 * l + (vi - (16 * A + 12))] = t;
        }
    }
    if (threadIdx.x < 2 * A + 3) {
        const int i = threadIdx.x;
        const float t = redb[i];
        if (i < A) o[MUB + i] = t;
        else if (i < 2 * A) o[SGB + (i - A)] = t;
        else if (i == 2 * A) o[V3 + 256] = t;
        else o[V3 + 257 + (i - 2 * A - 1)] = t;      // the two loss-term partial sums close the heads' part of the row
    }
}

// (accumulate_loss_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)

// ------------------------------------------------------------------------------------------ loss scale
// The backward GEMMs run on the fp16 matrix pipe (net_gemm.h), whose operands must sit in 2^-14 .. 65504, and the head
// gradients are O(advantage / samples): ~1e-7 at 32 768 envs x 20 steps.  The backward pass is linear in them, so they are
// multiplied by a power of two S (exact in fp32) chosen per gradient pass from the largest |d loss / d z| of any head of
// any sample of the pass, and the finished flat gradient is multiplied by 1/S (exact): the result is what the unscaled
// pass would give, with every intermediate inside the fp16 range.  bound[0] = the bits of max over rows of
// max(|zm|, |zs|, |zv|) * samples (non-negative floats order like their bit patterns; atomicMax is order-independent).
template <int A>
__global__ __launch_bounds__(256) void head_bound_kernel(const float *__restrict__ mu, const float *__restrict__ sigma,
                                                         const float *__restrict__ vs, const float *__restrict__ actions,
                                                         const float *__restrict__ adv, const float *__restrict__ y, long n, float scale,
                                                         float beta, unsigned *__restrict__ bound) {
    // grid-stride over the rows, ONE atomic per workgroup: a wave per 64 rows with an atomic each was 102 400 atomics on one address
    // at 32 768 envs x 20 steps -- 1.2 ms on the main stream before the lanes fork, with nothing else in flight (round 5: 296 -> ~20 us
    // per 1.6 M rows)
    __shared__ float wmax[4];
    float b = 0.f;
    for (long row = (long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long)gridDim.x * 256) {
        const float Adv = adv[row], v = vs[row], tgt = y[row];
        float r = 0.f;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float m = mu[(size_t)row * A + a], s = sigma[(size_t)row * A + a], d = actions[(size_t)row * A + a] - m;
            const float dmu = -Adv * d / (s * s);
            const float dsg = -Adv * (d * d / (s * s * s) - 1.0f / s) - beta / s;
            r = fmaxf(r, fmaxf(fabsf(dmu * (1.0f - m * m)), fabsf(dsg * s * (1.0f - s))));
        }
        r = fmaxf(r, fabsf(0.5f * (v - tgt) * expm1f(v / scale)));
        if (!(r <= 3.0e38f)) r = 3.0e38f;      // inf / nan rows: the pass is lost anyway, keep the scale finite
        b = fmaxf(b, r);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = fmaxf(b, __shfl_xor(b, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        b = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (b > 0.f) atomicMax(bound, __float_as_uint(b));
    }
}

// lscale[0] = S = 2^k with S * bound * inv_total in (2^5, 2^6]: a factor 1000 of headroom below 65504 for what the
// layers' transposed weights can add, full fp16 precision down to 2^-20 of the largest head gradient; lscale[1] = 1/S
__global__ void loss_scale_kernel(const unsigned *__restrict__ bound, float inv_total, int enabled, float *__restrict__ lscale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float u = __uint_as_float(bound[0]) * inv_total;
    int k = 0;
    if (enabled && u > 0.f && u <= 3.0e38f) {
        int e;
        (void)frexpf(u, &e);      // u = f * 2^e, f in [0.5, 1)
        k = 6 - e;
        k = k < -96 ? -96 : (k > 96 ? 96 : k);
    }
    lscale[0] = ldexpf(1.0f, k);
    lscale[1] = ldexpf(1.0f, -k);
}

__global__ void unscale_grads_kernel(float *__restrict__ g, long n, const float *__restrict__ lscale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] *= lscale[1];
}

// ------------------------------------------------------------------------------------------ weight rearrangement
// w3t[ci][(ty,tx,co)] = W3[2-ty][2-tx][ci][co]           (data gradient of conv3 as a gather; [N][K] for gemm_rowk)
// w2t[py*2+px][ci][(ty,tx,co)] = W2[py+2(1-ty)][px+2(1-tx)][ci][co]   (conv2, one matrix per pixel parity)
__global__ void transpose_conv_weights_kernel(const float *__restrict__ w2, const float *__restrict__ w3, float *__restrict__ w2t,
                                              float *__restrict__ w3t) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 576 * 64) {
        int ci = i & 63, r = i >> 6;
        int co = r & 63, t = r >> 6, ty = t / 3, tx = t - ty * 3;
        w3t[ci * 576 + r] = w3[(((2 - ty) * 3 + (2 - tx)) * 64 + ci) * 64 + co];
    }
    if (i < 4 * 256 * 32) {
        int ci = i & 31, r = i >> 5;
        int co = r & 63, t = (r >> 6) & 3, cls = r >> 8;
        int ty = t >> 1, tx = t & 1, py = cls >> 1, px = cls & 1;
        int ky = py + 2 * (1 - ty), kx = px + 2 * (1 - tx);
        w2t[(cls * 32 + ci) * 256 + (r & 255)] = w2[((ky * 4 + kx) * 32 + ci) * 64 + co];
    }
}

// ------------------------------------------------------------------------------------------ conv1 weight gradient
// dW1[ky][kx][c][co] = sum_samples sum_{nonzero pixel (h,w,c,val)} val * ga1[sample][oy][ox][co], (h,w) = (4oy+ky, 4ox+kx).
// Channels 0/1 are shared by an env's 10 agents, so their ga1 are summed first.  Each block walks a
// strided set of envs with float64 LDS accumulators and writes one partial to slab64[block][6144].
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const uint8_t *__restrict__ lbins, const uint8_t *__restrict__ abins,
                                                          const uint8_t *__restrict__ pos, const float *__restrict__ ga1,
                                                          int nenv, int G, double *__restrict__ slab64, const float *__restrict__ ds) {
    __shared__ double acc[6144];
    __shared__ float gsum[400 * 32];
    __shared__ unsigned int cnt[2][7056 / 4 + 4];
    __shared__ int nz_list[96];      // packed: h | w<<8 | c<<16 | count<<20
    __shared__ int nz_n;
    const int tid = threadIdx.x;
    for (int i = tid; i < 6144; i += 256) acc[i] = 0.0;
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        for (int i = tid; i < 2 * (7056 / 4 + 4); i += 256) (&cnt[0][0])[i] = 0;
        if (tid == 0) nz_n = 0;
        for (int i = tid; i < 3200; i += 256) {     // sum of the 10 agents' gradients (shared-trunk mode: dS is that sum already)
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ds) {
                s = reinterpret_cast<const float4 *>(ds + (size_t)env * 12800)[i];
            } else {
                for (int a = 0; a < 10; ++a) {
                    float4 v = reinterpret_cast<const float4 *>(ga1 + ((size_t)env * 10 + a) * 12800)[i];
                    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                }
            }
            reinterpret_cast<float4 *>(gsum)[i] = s;
        }
        __syncthreads();
        int my_idx = -1, my_c = 0;
        if (tid < 90) {
            const uint8_t *b = tid < 80 ? lbins + ((size_t)env * 80 + tid) * 2 : abins + ((size_t)env * 10 + (tid - 80)) * 2;
            my_c = tid < 80 ? 0 : 1;
            if (b[0] != 255) {
                my_idx = b[0] * G + b[1];
                atomicAdd(&cnt[my_c][my_idx >> 2], 1u << (8 * (my_idx & 3)));
            }
        }
        __syncthreads();
        if (my_idx >= 0) {     // the lowest point id in a bin lists it (unique list, deterministic content)
            bool first = true;
            const uint8_t *base = my_c == 0 ? lbins + (size_t)env * 160 : abins + (size_t)env * 20;
            int me = my_c == 0 ? tid : tid - 80;
            for (int j = 0; j < me; ++j)
                if (base[j * 2] != 255 && base[j * 2] * G + base[j * 2 + 1] == my_idx) { first = false; break; }
            if (first) {
                unsigned int k = (cnt[my_c][my_idx >> 2] >> (8 * (my_idx & 3))) & 255u;
                int slot = atomicAdd(&nz_n, 1);
                nz_list[slot] = (my_idx / G) | ((my_idx % G) << 8) | (my_c << 16) | ((int)k << 20);
            }
        }
        __syncthreads();
        const int nnz = nz_n;
        // shared channels: (nonzero, cover, co) items
        for (int it = tid; it < nnz * 4 * 32; it += 256) {
            int co = it & 31, cov = (it >> 5) & 3, z = it >> 7;
            int e = nz_list[z];
            int hh = e & 255, ww = (e >> 8) & 255, c = (e >> 16) & 15, k = e >> 20;
            int oy = hh / 4 - (cov >> 1), ox = ww / 4 - (cov & 1);
            int ky = hh - 4 * oy, kx = ww - 4 * ox;
            if (oy >= 0 && oy < 20 && ox >= 0 && ox < 20 && ky < 8 && kx < 8) {
                float val = (float)((double)k / (c == 0 ? 80.0 : 10.0));
                atomicAdd(&acc[((ky * 8 + kx) * 3 + c) * 32 + co], (double)(val * gsum[(oy * 20 + ox) * 32 + co]));
            }
        }
        // one-hot channel: (agent, cover, co) items (shared-trunk mode: done by agent_corr_backward_kernel)
        for (int it = tid; it < (ds ? 0 : 10 * 4 * 32); it += 256) {
            int co = it & 31, cov = (it >> 5) & 3, a = it >> 7;
            int hh = pos[((size_t)env * 10 + a) * 2], ww = pos[((size_t)env * 10 + a) * 2 + 1];
            int oy = hh / 4 - (cov >> 1), ox = ww / 4 - (cov & 1);
            int ky = hh - 4 * oy, kx = ww - 4 * ox;
            if (oy >= 0 && oy < 20 && ox >= 0 && ox < 20 && ky < 8 && kx < 8)
                atomicAdd(&acc[((ky * 8 + kx) * 3 + 2) * 32 + co], (double)ga1[((size_t)env * 10 + a) * 12800 + (oy * 20 + ox) * 32 + co]);
        }
    }
    __syncthreads();
    for (int i = tid; i < 6144; i += 256) slab64[(size_t)blockIdx.x * 6144 + i] = acc[i];
}

// Shared-trunk form: only the two count channels (the one-hot channel is folded by agent_ds_kernel), dS read straight from
// global memory.  conv1's stride is 4 and its kernel 8 x 8, so a non-zero input pixel (h, w) meets exactly four output pixels
// ("covers" (dy, dx): oy = h/4 - dy, ox = w/4 - dx) and in cover (dy, dx) only the kernel tap (h%4 + 4 dy, w%4 + 4 dx).
// A thread = (q = (h%4, w%4), channel pair): it owns the 4 covers x 2 input channels x 2 output channels of its q in REGISTERS
// (16 doubles) and walks only the env's bins with that q -- 1/16 of them on average -- with the four covers' dS loads of kWgBins bins
// in flight together.  The bins of an env are bucketed by (input channel, q) in point order with wave ballots.  No atomics, and
// the order of additions per accumulator is fixed: bins by their lowest point id, envs in the workgroup's stride order, workgroups
// reduced in index order (slab64_reduce_shared_kernel) -- bitwise reproducible, and the same sums in the same order as the first
// version of this kernel (a thread per (cover, channel, output channel) walking ALL bins of the env with its 16 q-accumulators in
// LDS: 231 us per 8 192-env chunk, an 80-step serial chain per env).
constexpr int kWgBins = 2;      // 4 measured no faster: the per-env set-up, not the walk, is what is left
__global__ __launch_bounds__(256, 6) void conv1_wgrad_shared_kernel(const uint8_t *__restrict__ lbins, const uint8_t *__restrict__ abins,
                                                                 const float *__restrict__ ds, int nenv, int G,
                                                                 double *__restrict__ slab64) {
    __shared__ int bins[96];            // bin index h*G + w of point i (locusts 0..79, agents 80..89), -1 = outside
    __shared__ int blist[2][16][80];    // per (input channel, q): packed h | w<<8 | count<<20 of its listed bins, in point order
    __shared__ int bcnt[2][16], w0cnt[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = tid >> 4, cp = tid & 15;      // this thread's tap class and output channels 2 cp, 2 cp + 1
    double acc[4][2][2];
#pragma unroll
    for (int i = 0; i < 16; ++i) (&acc[0][0][0])[i] = 0.0;
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        __syncthreads();
        if (tid < 90) {
            const uint8_t *b = tid < 80 ? lbins + ((size_t)env * 80 + tid) * 2 : abins + ((size_t)env * 10 + (tid - 80)) * 2;
            bins[tid] = b[0] != 255 ? b[0] * G + b[1] : -1;
        }
        __syncthreads();
        bool first = false;
        int k = 0, myq = -1, mine = -1;
        if (tid < 90 && bins[tid] >= 0) {     // the lowest point id in a bin lists it with the bin's count
            const int lo = tid < 80 ? 0 : 80, hi = tid < 80 ? 80 : 90;
            mine = bins[tid];
            first = true;
            for (int j = lo; j < hi; ++j) {
                const bool same = bins[j] == mine;
                k += same ? 1 : 0;
                first = first && !(same && j < tid);
            }
            myq = ((mine / G) & 3) * 4 + ((mine % G) & 3);
        }
        // bucket position = listed points of the same (channel, q) with a lower point id: ballots per q (wave 0: points 0..63, wave 1: 64..89)
        int pos = 0;
        if (tid < 128) {
            const unsigned long long below = (1ull << lane) - 1ull;
            const bool loc = first && tid < 80, agt = first && tid >= 80;
#pragma unroll
            for (int qq = 0; qq < 16; ++qq) {
                const unsigned long long ml = __ballot(loc && myq == qq), ma = __ballot(agt && myq == qq);
                if (myq == qq) pos = __popcll((loc ? ml : ma) & below);
                if (tid == 0) w0cnt[qq] = __popcll(ml);
                if (tid == 64) { bcnt[0][qq] = __popcll(ml); bcnt[1][qq] = __popcll(ma); }      // wave 1's share; wave 0's is added below
            }
        }
        __syncthreads();
        if (tid < 128) {
            if (first) {
                const int c = tid < 80 ? 0 : 1, at = pos + ((tid >= 64 && tid < 80) ? w0cnt[myq] : 0);
                blist[c][myq][at] = (mine / G) | ((mine % G) << 8) | (k << 20);
            }
            if (tid >= 64 && tid < 80) bcnt[0][tid - 64] += w0cnt[tid - 64];
        }
        __syncthreads();
        const float *dsenv = ds + (size_t)env * 12800 + 2 * cp;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int nb = bcnt[c][q];
            const double inv = c == 0 ? 80.0 : 10.0;
            for (int z0 = 0; z0 < nb; z0 += kWgBins) {      // kWgBins bins x four covers of 8-byte loads in flight, then added in list order
                float2 v[kWgBins][4];
                bool okc[kWgBins][4];
                float val[kWgBins];
#pragma unroll
                for (int u = 0; u < kWgBins; ++u) {
                    const int z = z0 + u;
                    const int e = blist[c][q][z < nb ? z : z0];
                    const int hh = e & 255, ww = (e >> 8) & 255, kk = e >> 20;
                    val[u] = (float)((double)kk / inv);
#pragma unroll
                    for (int cov = 0; cov < 4; ++cov) {
                        const int oy = hh / 4 - (cov >> 1), ox = ww / 4 - (cov & 1);
                        okc[u][cov] = z < nb && oy >= 0 && oy < 20 && ox >= 0 && ox < 20;
                        v[u][cov] = *reinterpret_cast<const float2 *>(dsenv + (okc[u][cov] ? oy * 20 + ox : 0) * 32);
                    }
                }
#pragma unroll
                for (int u = 0; u < kWgBins; ++u)
#pragma unroll
                    for (int cov = 0; cov < 4; ++cov)
                        if (okc[u][cov]) {
                            acc[cov][c][0] += (double)(val[u] * v[u][cov].x);
                            acc[cov][c][1] += (double)(val[u] * v[u][cov].y);
                        }
            }
        }
    }
    // slab layout [tap = ky*8 + kx][c][co] with ky = h%4 + 4 dy, kx = w%4 + 4 dx
#pragma unroll
    for (int cov = 0; cov < 4; ++cov) {
        const int ky = (q >> 2) + 4 * (cov >> 1), kx = (q & 3) + 4 * (cov & 1);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) slab64[(size_t)blockIdx.x * 4096 + ((ky * 8 + kx) * 2 + c) * 32 + 2 * cp + j] = acc[cov][c][j];
    }
}

// The same sums from the env's index record (obs_index_kernel, net_shared.inc): the bucket (channel, q) of this thread is a range of the
// record's list -- the 16 lanes of a q read one address -- so the per-env set-up above (three barriers, the duplicate scan, the ballots,
// 10.7 KB of LDS) is gone and nothing in the kernel waits for another wave.  The next env's bucket ranges and the first kWgBins entries of
// each bucket are requested before the current env is walked.  Order of additions per accumulator as above (bins by lowest point id,
// envs in stride order, workgroups in index order): launched on the same grid, it writes the same slabs bit for bit.
// 117 -> 77 us per 8 192-env chunk (single stream); what is left is the chain list entry -> dS rows -> adds of the ~5 envs of a workgroup.
struct WgradBuckets {
    unsigned range;      // lo | hi << 8 of channel 0's bucket, << 16 of channel 1's
    unsigned e[2][kWgBins];
};
__device__ __forceinline__ WgradBuckets wgrad_fetch(const unsigned *__restrict__ rec, int env, int nenv, int q) {
    WgradBuckets b;
    const unsigned *r = rec + (size_t)(env < nenv ? env : nenv - 1) * kObsWords;
    const uint8_t *off = reinterpret_cast<const uint8_t *>(r + kObsOff);
    b.range = 0u;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const unsigned lo = off[c * 16 + q], hi = env < nenv ? off[c * 16 + q + 1] : lo;
        b.range |= (lo | (hi << 8)) << (16 * c);
#pragma unroll
        for (int u = 0; u < kWgBins; ++u) b.e[c][u] = lo + u < hi ? r[kObsList + lo + u] : 0u;
    }
    return b;
}
__global__ __launch_bounds__(256, 6) void conv1_wgrad_indexed_kernel(const unsigned *__restrict__ rec, const float *__restrict__ ds, int nenv,
                                                                  double *__restrict__ slab64) {
    const int tid = threadIdx.x;
    const int q = tid >> 4, cp = tid & 15;      // this thread's tap class and output channels 2 cp, 2 cp + 1
    double acc[4][2][2];
#pragma unroll
    for (int i = 0; i < 16; ++i) (&acc[0][0][0])[i] = 0.0;
    WgradBuckets nx = wgrad_fetch(rec, blockIdx.x, nenv, q);
    for (int env = blockIdx.x; env < nenv; env += gridDim.x) {
        const WgradBuckets cur = nx;
        nx = wgrad_fetch(rec, env + gridDim.x, nenv, q);
        const unsigned *list = rec + (size_t)env * kObsWords + kObsList;
        const float *dsenv = ds + (size_t)env * 12800 + 2 * cp;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int lo = (cur.range >> (16 * c)) & 255, nb = (int)((cur.range >> (16 * c + 8)) & 255) - lo;
            const double inv = c == 0 ? 80.0 : 10.0;
            unsigned en[kWgBins];
#pragma unroll
            for (int u = 0; u < kWgBins; ++u) en[u] = cur.e[c][u];
            for (int z0 = 0; z0 < nb; z0 += kWgBins) {      // kWgBins bins x four covers of 8-byte loads in flight, then added in list order
                float2 v[kWgBins][4];
                bool okc[kWgBins][4];
                float val[kWgBins];
                int ec[kWgBins];
#pragma unroll
                for (int u = 0; u < kWgBins; ++u) {      // ... and the next group's entries requested beside them
                    ec[u] = (int)en[u];
                    en[u] = z0 + kWgBins + u < nb ? list[lo + z0 + kWgBins + u] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kWgBins; ++u) {
                    const int z = z0 + u;
                    const int e = ec[u];
                    const int hh = e & 255, ww = (e >> 8) & 255, kk = e >> 20;
                    val[u] = (float)((double)kk / inv);
#pragma unroll
                    for (int cov = 0; cov < 4; ++cov) {
                        const int oy = hh / 4 - (cov >> 1), ox = ww / 4 - (cov & 1);
                        okc[u][cov] = z < nb && oy >= 0 && oy < 20 && ox >= 0 && ox < 20;
                        v[u][cov] = *reinterpret_cast<const float2 *>(dsenv + (okc[u][cov] ? oy * 20 + ox : 0) * 32);
                    }
                }
#pragma unroll
                for (int u = 0; u < kWgBins; ++u)
#pragma unroll
                    for (int cov = 0; cov < 4; ++cov)
                        if (okc[u][cov]) {
                            acc[cov][c][0] += (double)(val[u] * v[u][cov].x);
                            acc[cov][c][1] += (double)(val[u] * v[u][cov].y);
                        }
            }
        }
    }
    // slab layout [tap = ky*8 + kx][c][co] with ky = h%4 + 4 dy, kx = w%4 + 4 dx
#pragma unroll
    for (int cov = 0; cov < 4; ++cov) {
        const int ky = (q >> 2) + 4 * (cov >> 1), kx = (q & 3) + 4 * (cov & 1);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) slab64[(size_t)blockIdx.x * 4096 + ((ky * 8 + kx) * 2 + c) * 32 + 2 * cp + j] = acc[cov][c][j];
    }
}

// (slab64_reduce_shared_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)

__global__ void slab64_reduce_kernel(const double *__restrict__ slab, int chunks, int n, float *__restrict__ dst) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += slab[(size_t)c * n + i];
    dst[i] += (float)s;
}

// ------------------------------------------------------------------------------------------ optimiser
// stats[0..1] = loss parts (mean), stats[2] = loss, stats[3] = global_norm, stats[4] = clip factor
__global__ void finalize_stats_kernel(const double *__restrict__ partial, int nparts, const double *__restrict__ stats64,
                                      float inv_total, float clip_norm, float grad_scale, float *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += partial[i];
    float norm = (float)(sqrt(s) * (double)grad_scale);
    float pl = (float)(stats64[0] * (double)inv_total), cl = (float)(stats64[1] * (double)inv_total);
    stats[0] = pl; stats[1] = cl; stats[2] = pl + cl; stats[3] = norm;
    // tf.clip_by_global_norm: g * clip_norm / max(global_norm, clip_norm)   (actor_learner.py:52-57)
    stats[4] = grad_scale * (clip_norm > 0.f ? clip_norm / fmaxf(norm, clip_norm) : 1.0f);
}

// after Adam: the flag of the gradient pass (what Adam just looked at) moves into the net's latch word and the device flag starts
// from zero for what follows -- the background pass of refresh_transposes runs fp16 GEMMs on the UPDATED parameters, and a flag
// raised there says nothing about the update that was just applied (train_apply)
__global__ void range_latch_kernel(int *flag, int *latch) {
    *latch = *flag;
    *flag = 0;
}

// end of a rollout: a range flag raised by ITS forward passes becomes 3, so that the gradient step (which reads the flag at its
// synchronisation point, max-reduced over the ranks) can tell "the rollout itself is invalid" from "only my backward pass overflowed"
__global__ void rollout_range_mark_kernel(int *flag) {
    if (*flag) *flag = 3;
}

// rewards[t] of the envs [e0, e0 + ne).  layout 0: every agent column of the env gets its reward; layout 1: rewards[t, e_idx] = r_e
// for e_idx < E only (paac.py:289,331-338: a (T, E*10) array indexed by env id -- quirk Q4; the columns >= E stay at the zeros
// grl_net_rollout fills the buffer with)
__global__ void reward_layout_kernel(const float *__restrict__ reward, int e0, int ne, int layout, float *__restrict__ out,
                                     const uint8_t *__restrict__ done, uint8_t *__restrict__ ro_done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ne) ro_done[e0 + i] = done[e0 + i];      // dones[t] of the chunk's envs ride along (a copy of its own until round 3)
    if (layout == 0) {
        if (i < ne * 10) out[(size_t)e0 * 10 + i] = reward[e0 + i / 10];
    } else if (i < ne) {
        out[e0 + i] = reward[e0 + i];
    }
}

// ------------------------------------------------------------------------------------------ host side
struct TrainBufs {
    float *cmu, *csigma, *cvs, *dzh, *cact, *cadv, *cy;
    double *stats64, *partial;
};

// gradient-step workspace of the lane currently loaded into *net
static int ensure_train_bufs(grl_net *net) {
    if (net->train_ready) return GRL_OK;
    size_t c = net->chunk;
    int rc = GRL_OK;
    auto A = [&](auto **p, size_t cnt) { if (rc == GRL_OK) rc = paac_alloc(net, p, cnt); };
    if (!net->shared_trunk) { A(&net->ga1, c * 12800); A(&net->ga2, c * 5184); A(&net->ga3, c * 3136); }
    A(&net->gd1, c * 512); A(&net->gd2, c * 256); A(&net->gp1, c * 512 * 2); net->gv1 = net->gp1 + c * 512; A(&net->gv2, c * 256);
    if (!net->w3t) { A(&net->w3t, 576 * 64); A(&net->w2t, 4 * 256 * 32); }      // shared by the lanes (read-only during a pass)
    A(&net->dz2, (c / 10) * 5184); A(&net->gt, (c / 10) * 12800);
    A(&net->gsl, c * 9 * 64); A(&net->dza, c * 9 * 64); A(&net->dz3sh, (c / 10) * 3136); A(&net->tmpw3, 576 * 64);
    A(&net->t2desc, (size_t)4 * net->npad);
    A(&net->dl2, (size_t)4 * net->npad * 32); A(&net->tt2, (size_t)4 * net->npad * 32);
    A(&net->tmpw2, 4 * 256 * 32);
    A(&net->gd1sh, (c / 10) * 512); A(&net->gsh3, (c / 10) * 3136); A(&net->g3p, c * 1600); A(&net->dz3p, c * 1600);
    // every producer of a chunk keeps its own region until the chunk's queued reductions run (net_reduce.inc): the dense1 patch
    // slices (the largest: pslices x 1600 x 512) plus ~70 M floats for the other weight gradients of a full-size chunk
    // (+ 32 M since round 5: conv3's slot weight gradient runs over up to 684 row ranges of 576 x 64; a buffer that fills up mid-chunk
    // flushes the queue early -- seven reduction launches per chunk instead of four)
    net->slab_floats = ((size_t)112 << 20) + (size_t)net->pslices * 1600 * 512;
    A(&net->slab, net->slab_floats);
    net->slab_used = 0;
    A(&net->slab1h, (size_t)2048 * 2048);
    {   // column sums per wave tile of a dgrad GEMM: the dense stack's (128-row tiles, kW128M wave tiles, 512 columns), conv2's transposed
        // convolution (128 columns over env * 100 rows), conv3's over the affected conv2 rows (128-row tiles, 4 wave tiles, 64 columns)
        size_t sb = ((size_t)c / 128 + 2) * kW128M * 512;
        sb = std::max(sb, ((size_t)(c / 10) * 100 / 128 + 2) * kW128M * 128);
        sb = std::max(sb, ((size_t)(c / 10) * 81 / 128 + 2) * 4 * 64);
        net->slabb_floats = 5 * sb + 4096;      // the three dense data gradients and the conv ones of a chunk side by side
        A(&net->slabb, net->slabb_floats);
        net->slabb_used = 0;
    }
    A(&net->slab1b, (size_t)3 * 2048 * 64);      // agent_dz3, agent_dz2, agent_ds: a region each
    A(&net->cfold, (size_t)kFoldParts * 32);
    A(&net->slab64, kSlab64Doubles + 4096);
    A(&net->ro_mu, c * (3 * (size_t)net->ho.A + net->ho.dz + 3));      // cmu csigma cvs dzh cact cadv cy
    if (rc == GRL_OK) net->train_ready = true;
    return rc;
}

template <int BM, int BN, int WGM, int WGN, class AG>
static int tn_launch(grl_net *net, int rd, AG ag, int I, const float *dY, int J, float *gdst, int accumulate = 1, double flop_rows = 0.0,
                     int min_chunks = 0, int wgs = 0) {
    const int M = ag.rows;
    const long n = (long)I * J;
    int chunks, mc;
    float *slab = slab_plan_take(net, wgs > 0 ? wgs : net->tn_wgs, (I / BM) * (J / BN), min_chunks, M, (size_t)n, "tn_launch: slab too small", &chunks, &mc);
    if (!slab) return GRL_E_INVALID;
    {
        GemmTimer t(net, 2.0 * (flop_rows > 0.0 ? flop_rows : (double)M) * (double)I * J);
        launch_tn<BM, BN, WGM, WGN, AG>(net, dim3(I / BM, J / BN, chunks), net->h->stream, ag, dY, J, mc, slab);
    }
    RJob j{};
    j.kind = RJ_SLAB; j.blocks = (int)((n + 255) / 256); j.i0 = chunks; j.i1 = accumulate; j.n = n; j.p0 = slab; j.d0 = gdst;
    rq_push(net, rd, j);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// conv3's per-slot weight-gradient correction (SlotGatherT3P^T . d2s over the tap-class sorted slot rows): tn_launch with the live-tap
// union of every row range, so that gemm_tn writes no slab tile for the taps a range does not have and the reduction skips the same
__global__ __launch_bounds__(256) void slot_range_masks_kernel(const int *__restrict__ sperm, const unsigned short *__restrict__ stap,
                                                               const int *__restrict__ live, int mc, unsigned *__restrict__ zmask) {
    __shared__ unsigned part[4];
    const int beg = blockIdx.x * mc, end = min(*live, beg + mc);
    unsigned v = 0;
    for (int s = beg + threadIdx.x; s < end; s += 256) v |= stap[sperm[s]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) zmask[blockIdx.x] = part[0] | part[1] | part[2] | part[3];
}
// (slab_reduce_taps_kernel: its body is a job of reduce_batch_kernel since round 4, net_reduce.inc)
static int slot_wgrad_launch(grl_net *net, int n, float *gw3, double flop_rows, int min_chunks) {
    constexpr int BM = 64, BN = 64, I = 576, J = 64;
    const int M = n * 9;
    if (net->swgrad_chunks > 0) min_chunks = net->swgrad_chunks;
    int chunks, mc;
    float *slab = slab_plan_take(net, net->tn_wgs, (I / BM) * (J / BN), min_chunks, M, (size_t)I * J, "slot_wgrad_launch: slab too small", &chunks, &mc);
    if (!slab) return GRL_E_INVALID;
    hipStream_t st = net->h->stream;
    const bool skip = net->patch_skip != 0;
    if (skip) hipLaunchKernelGGL(slot_range_masks_kernel, dim3(chunks), dim3(256), 0, st, net->sperm, net->stap, net->sbase + n, mc, net->szmask);
    SlotGatherT3P ag{net->dz3p, net->rowdesc, M, net->sbase + n, net->sperm, nullptr, skip ? net->szmask : nullptr};
    {
        GemmTimer t(net, 2.0 * flop_rows * (double)I * J * net->sfrac);
        if (net->swgrad_pair) {      // two live taps of the row range per 128-wide I tile: five tiles cover any tap set
            SlotGatherT3PPair gp{ag};
            launch_tn<128, BN, 2, 2, SlotGatherT3PPair>(net, dim3(5, J / BN, chunks), st, gp, net->d2s, J, mc, slab);
        } else
            launch_tn<BM, BN, 2, 2, SlotGatherT3P>(net, dim3(I / BM, J / BN, chunks), st, ag, net->d2s, J, mc, slab);
    }
    // the masked sum over the row ranges and conv3_corr_add's tap flip in one queued job (net_reduce.inc)
    RJob j{};
    j.kind = RJ_TAPS_C3; j.blocks = I * J / 32; j.i0 = chunks; j.p0 = slab; j.p1 = skip ? net->szmask : nullptr; j.d0 = gw3;
    rq_push(net, RD_C3W, j);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

static int colsum_launch(grl_net *net, int rd, const float *dY, int M, int J, float *gdst) {
    if (J < 32 || J > 1024 || (J & (J - 1))) return paac_fail(net, GRL_E_INVALID, "colsum_launch: J must be a power of two in 32..1024");
    int chunks = (M + 31) / 32;
    if (chunks > 2048) chunks = 2048;
    int mc = (M + chunks - 1) / chunks;
    chunks = (M + mc - 1) / mc;
    float *slab = slab_take(net, (size_t)chunks * J);
    if (!slab) return paac_fail(net, GRL_E_INVALID, "colsum_launch: slab too small");
    hipLaunchKernelGGL(colsum_kernel, dim3(1, chunks), dim3(256), 0, net->h->stream, dY, M, J, mc, slab);
    RJob j{};
    j.kind = RJ_NARROW; j.blocks = (J + kNarrowCols - 1) / kNarrowCols; j.i0 = chunks; j.i1 = 1; j.n = J; j.p0 = slab; j.d0 = gdst;
    rq_push(net, rd, j);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// bias gradient from the per-wave-tile column sums an EpiGradSum GEMM (128-row tiles, kW128M wave tiles each) left in slabb
static void csum_reduce(grl_net *net, int rd, const float *csum, int rows, int J, float *bias_dst) {
    const int parts = (rows + 127) / 128 * kW128M;
    RJob j{};
    j.kind = RJ_NARROW; j.blocks = (J + kNarrowCols - 1) / kNarrowCols; j.i0 = parts; j.i1 = 1; j.n = J; j.p0 = csum; j.d0 = bias_dst;
    rq_push(net, rd, j);
}

template <int BM, int BN, int WGM, int WGN, bool FENCE = true, int NBUF = 1, bool ACC1 = false, class AG, class Epi>
static void rowk_launch(grl_net *net, AG ag, const float *W, int ldb, int N, Epi epi, double flops) {
    GemmTimer t(net, flops);
    launch_rowk<BM, BN, WGM, WGN, AG, Epi, true, FENCE, NBUF, ACC1>(net, dim3(N / BN, (ag.rows + BM - 1) / BM), net->h->stream, ag, W, ldb, N, epi);
}

// Workgroups of a 256-thread kernel that fit the device at once (occupancy x CUs), capped by what its partial-sum slab holds: the
// env-strided helper kernels are launched with exactly one resident wave of workgroups -- a grid of 2 048 on 1 536 resident slots
// runs a second, one-third-full wave (agent_dz3 327 -> 272 us, agent_dz2 220 -> 161, agent_ds 104 -> 80 per 8 192-env chunk).
static int resident_grid(const void *kernel, int cap) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipGetDeviceProperties(&prop, dev) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return cap;
    }
    // (round 5: half or a third of that wave, so that a waiting helper leaves wave slots and registers to the other lanes' GEMMs, moved the
    // four-stream update by less than the run-to-run spread: 301.9 / 296.4 against 305.7 / 297.3 ms at 50 %, 303.6 / 298.1 against 304.8 / 297.4 at 34 %)
    const long g = (long)per_cu * prop.multiProcessorCount;
    return g < cap ? (int)g : cap;
}

// forward + backward of one chunk; gradients are ACCUMULATED into net->grads.  slot >= 0: conv3 and the dense
// stack of this chunk are resident from the rollout (bind_activations) and are not recomputed.
static int backward_chunk_body(grl_net *net, const TrainBufs &tb, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv,
                               const float *actions, const float *adv, const float *y, float inv_total, long slot,
                               const float *pmu, const float *psg, const float *pval);
// The queue of deferred reductions and the bump pointers of their source regions live in *net and are shared by the lanes: nothing of
// them may outlive a chunk.  A chunk that fails half way (any early return below) would otherwise leave jobs pointing at slab
// regions the next chunk -- possibly of another lane -- allocates over and then flushes into its gradient (advisor r4).
static void rq_reset(grl_net *net) {
    net->rq.clear(); net->rq_dst.clear();
    net->slab_used = 0; net->slabb_used = 0;
}
static int backward_chunk(grl_net *net, const TrainBufs &tb, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv,
                          const float *actions, const float *adv, const float *y, float inv_total, long slot = -1,
                          const float *pmu = nullptr, const float *psg = nullptr, const float *pval = nullptr) {
    if (!net->rq.empty() || net->slab_used || net->slabb_used) {      // cannot happen: every exit below leaves them empty
        rq_reset(net);
        return paac_fail(net, GRL_E_INVALID, "backward_chunk: reductions of an earlier chunk were still queued");
    }
    const int rc = backward_chunk_body(net, tb, lb, ab, pos, nenv, actions, adv, y, inv_total, slot, pmu, psg, pval);
    if (rc != GRL_OK) rq_reset(net);
    return rc;
}
// ---- the stages of a chunk's backward pass, in the order backward_chunk_body runs them.  What every stage works on:
struct BwdCtx {
    grl_net *net;
    hipStream_t st;
    const float *P;      // parameters
    float *Gr;           // the lane's gradient accumulator
    int n, nenv;         // agent-samples and envs of the chunk
    bool trunk;          // trunk_skip && expand2_gemm: the trunk's row lists exist (trunk_index ran in this chunk's forward_chunk)
};

// head data gradients AND head weights / biases (one slab row per workgroup).  Queues: RD_HEADS
static int bwd_heads(const BwdCtx &c, const TrainBufs &tb, const float *hmu, const float *hsg, const float *hvs, const float *actions,
                     const float *adv, const float *y, float inv_total) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    const HeadOff &ho = net->ho;
    const int HS = heads_slab(ho.A), NW = 1024 * ho.A + 2 * ho.A;      // NW: [muw|mub|sgw|sgb], contiguous in the flat vector
    int chunks = (n + 4 * kHeadRows - 1) / (4 * kHeadRows);
    if (chunks > 1024) chunks = 1024;
    const int HS2 = HS + 768;      // + the bias rows of pol1 (512) and v2 (256): column sums of gp1 / gv2, taken while they are written
    float *hslab = slab_take(net, (size_t)chunks * HS2);
    if (!hslab) return paac_fail(net, GRL_E_INVALID, "backward_chunk: slab too small for the heads");
    GRL_HEADS_DISPATCH(ho.A, hipLaunchKernelGGL(heads_backward_kernel<kA>, dim3(chunks), dim3(256), 0, st, net->p1, net->v2,
                                                hmu, hsg, hvs, actions, adv, y, P, ho, n, net->cfg.scale, net->cfg.entropy_beta, inv_total,
                                                (const float *)(net->stats + kLossScaleAt), net->gp1, net->gv2, tb.dzh, tb.stats64, hslab));
    {   // one queued job: the slab rows' column sums go straight to the head kernels / biases, pol1's and v2's biases and the loss sums
        RJob j{};
        j.kind = RJ_HEADS; j.blocks = (HS2 + kNarrowCols - 1) / kNarrowCols; j.i0 = chunks; j.i1 = NW; j.i2 = HS; j.i3 = HS2; j.p0 = hslab;
        j.d0 = Gr + ho.muw; j.p1 = Gr + ho.v3w; j.p2 = Gr + ConvOffsets::p1b; j.p3 = Gr + net->ho.v2b; j.d1 = tb.stats64;
        rq_push(net, RD_HEADS, j);
    }
    return GRL_OK;
}

// ---- data gradients (dY * W^T with the ReLU mask of the producing layer fused)
// the dense stack's, common to both trunks.  Queues: RD_V1B, RD_D2B, RD_D1B
static int bwd_dense_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    const HeadOff &ho = net->ho;
    const size_t csum_floats = ((size_t)n / 128 + 2) * kW128M * 512;
    float *cs1 = slabb_take(net, csum_floats), *cs2 = slabb_take(net, csum_floats), *cs3 = slabb_take(net, csum_floats);
    if (!cs1 || !cs2 || !cs3) return paac_fail(net, GRL_E_INVALID, "backward_chunk: column-sum buffer too small");
    // (round 5: the one-accumulator form on this instance and on dense2 / v2's forwards -- 122 -> 92 registers, no faster alone -- moved the
    // four-stream update by nothing: 300.2 / 301.2 / 299.7 / 301.9 against 302.9 / 300.4 / 300.7 / 300.2 ms)
    rowk_launch<128, 128, kW128M, kW128N>(net, DenseRows{net->gv2, n, 256, 256}, P + ho.v2w, 256, 512,
                                      EpiGradSumBits{net->gv1, 512, net->mb_v1, cs1}, 2.0 * n * 256 * 512);
    csum_reduce(net, RD_V1B, cs1, n, 512, Gr + ho.v1b);
    // gd2 = relu'(d2) . (gp1 . pol1_w^T + gv1 . v1_w^T) as ONE K = 1024 GEMM over [gp1 | gv1] and the two stacked kernels
    rowk_launch<128, 128, kW128M, kW128N, true, 2>(net, DenseRowsPair{net->gp1, n, 512, 512, (int)(net->gv1 - net->gp1), (int)(ho.v1w - ConvOffsets::p1w)},
                                P + ConvOffsets::p1w, 512, 256, EpiGradSumBits{net->gd2, 256, net->mb_d2, cs2}, 2.0 * n * 1024 * 256);
    csum_reduce(net, RD_D2B, cs2, n, 256, Gr + ConvOffsets::d2b);
    rowk_launch<128, 128, kW128M, kW128N>(net, DenseRows{net->gd2, n, 256, 256}, P + ConvOffsets::d2w, 256, 512,
                                      EpiGradSum{net->gd1, 512, net->d1, cs3}, 2.0 * n * 256 * 512);
    csum_reduce(net, RD_D1B, cs3, n, 512, Gr + ConvOffsets::d1b);
    return GRL_OK;
}

// the per-agent trunk (GRL_NET_F_PER_AGENT_TRUNK, the A/B reference): dense1, conv3 and conv2 on every agent's own rows.  Queues nothing
static int bwd_per_agent_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    rowk_launch<256, 64, kW256M, kW256N>(net, DenseRows{net->gd1, n, 512, 512}, P + ConvOffsets::d1w, 512, 3136,
                               EpiGrad{net->ga3, 3136, net->a3}, 2.0 * n * 512 * 3136);
    if (n % 256 == 0)     // pixel-major rows: taps outside the 7x7 image are skipped per workgroup (441 of 729 remain)
        rowk_launch<256, 64, 4, 1, false>(net, GatherT3PM{net->ga3, n * 81, n}, net->w3t, 576, 64, EpiGradPM{net->ga2, net->a2, n, 81, 64},
                                   2.0 * n * 441 * 64 * 64);
    else
        rowk_launch<256, 64, 4, 1, false>(net, GatherT3{net->ga3, n * 81}, net->w3t, 576, 64, EpiGrad{net->ga2, 64, net->a2},
                                   2.0 * n * 81 * 576 * 64);
    // w2t is [4 classes * 32 ci][256]: one N=128 GEMM, the gathered A tile is loaded once for all four classes
    rowk_launch<128, 128, 2, 2, false>(net, GatherT2{net->ga2, n * 100}, net->w2t, 256, 128, EpiGradStride2<true>{net->ga1, net->a1, nullptr},
                                2.0 * n * 100 * 256 * 128);
    return GRL_OK;
}

// dense1's data gradient on the shared a3 (net_patch.inc): all 3136 inputs once per env on the agent-summed gd1,
// the 1600 patch inputs per agent (group-sorted rows); the exact mask corrections follow in bwd_conv3_dgrad.  Queues nothing
static int bwd_dense1_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    hipLaunchKernelGGL(reduce_agents_kernel, dim3((unsigned)(((size_t)nenv * 128 + 255) / 256)), dim3(256), 0, st, net->gd1, nenv, 128,
                       net->gd1sh);
    net->prof_tag_cur = PT_ENV_DGRAD;
    if (trunk) {
        // only the pixels of the chunk's union mask; of the others nothing but the sum over the envs is used: G = column sums of
        // gd1sh, trunk_upix / trunk_uadd below (and the rank-1 rows of the weight gradient further down)
        int cch = (nenv + 31) / 32;
        if (cch > 2048) cch = 2048;
        const int cmc = (nenv + cch - 1) / cch;
        cch = (nenv + cmc - 1) / cmc;
        float *gslab = slab_take(net, (size_t)cch * 512);
        if (!gslab) return paac_fail(net, GRL_E_INVALID, "backward_chunk: slab too small");
        hipLaunchKernelGGL(colsum_kernel, dim3(1, cch), dim3(256), 0, st, (const float *)net->gd1sh, nenv, 512, cmc, gslab);
        hipLaunchKernelGGL(slab_reduce_narrow_kernel, dim3((512 + kNarrowCols - 1) / kNarrowCols), dim3(256), 0, st, gslab, cch, 512, net->tug, 0);
        rowk_launch<256, 64, kW256M, kW256N>(net, DenseRowsNU{{net->gd1sh, nenv, 512, 512}, net->tumask}, P + ConvOffsets::d1w, 512, 3136,
                                   EpiStore{net->gsh3, 3136}, 2.0 * nenv * 512 * 64.0 * trunk_union_pixels(net));
    } else {
        rowk_launch<256, 64, kW256M, kW256N>(net, DenseRows{net->gd1sh, nenv, 512, 512}, P + ConvOffsets::d1w, 512, 3136,
                                   EpiStore{net->gsh3, 3136}, 2.0 * nenv * 512 * 3136);
    }
    {
        PatchRows g{net->gd1, net->perm, net->tilegroup, net->ptiles * 256, 512, 512, 1, nullptr, nullptr, net->patch_skip ? net->tmask : nullptr, nullptr};
        net->prof_tag_cur = PT_PATCH_DGRAD;
        GemmTimer t(net, 2.0 * n * 512 * 1600 * net->pfrac[1]);
        if (net->pdgrad_pair) {      // two live pixels per 128-wide N tile: 13 tiles cover any support
            PatchRowsPairN gp{g};
            // (measured on this instance, round 5, interior / rim us per chunk: as is 339 / 139; without the scheduling fences 334 / 135; two
            // LDS buffers 331 / 134; launch order instead of the XCD-aware one 370 / 139; the one-accumulator form 848 / 333)
            launch_rowk<128, 128, kW128M, kW128N, PatchRowsPairN, EpiPermStore, true>(net, dim3(13, net->ptiles * 2), st, gp, P + ConvOffsets::d1w, 512, 1600,
                                                                                      EpiPermStore{net->g3p, net->perm, 1600});
        } else if (net->pdgrad_xcd)
            launch_rowk<256, 64, kW256M, kW256N, PatchRows, EpiPermStore, true>(net, dim3(1600 / 64, net->ptiles), st, g, P + ConvOffsets::d1w, 512, 1600, EpiPermStore{net->g3p, net->perm, 1600});
        else
            launch_rowk<256, 64, kW256M, kW256N, PatchRows, EpiPermStore, false>(net, dim3(1600 / 64, net->ptiles), st, g, P + ConvOffsets::d1w, 512, 1600, EpiPermStore{net->g3p, net->perm, 1600});
    }
    return GRL_OK;
}

// the exact mask corrections of dense1's data gradient -> DZ3 per env, dz3 per patch (agent_dz3), then conv3's data gradient on the
// shared a2.  Queues: RD_C3B (without the trunk skip; with it trunk_closed3_kernel adds conv3's bias gradient in bwd_slot_dgrad)
static int bwd_conv3_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    // (round 5: the same sums with every pixel of the env's map added up by its OWNER thread in agent order -- no LDS fold, one barrier
    // per env instead of thirteen, 60 registers, bit-identical -- measured 138 / 234 us per chunk (rim / interior) against 110 / 187:
    // this kernel moves ~0.5 / 1.0 GB per launch, most of it L2 / MALL hits the miss counters do not show, in 256-byte granules, and the
    // fold walks an agent's support in memory order where the owner form reads one granule per covering agent)
    static const int hg3 = resident_grid((const void *)agent_dz3_kernel, 2048);
    maybe_evict(net);
    hipLaunchKernelGGL(agent_dz3_kernel, dim3(nenv < hg3 ? nenv : hg3), dim3(256), 0, st, net->gsh3, net->g3p, net->a3sh, net->m3,
                       net->org, net->patch_skip ? net->smask : nullptr, nenv, net->dz3sh, net->dz3p, net->slab1b,
                       trunk ? (const unsigned *)net->tcmask : (const unsigned *)nullptr, trunk ? net->tslab + 2048 * 64 : (float *)nullptr,
                       trunk ? (const float *)(net->tbgz3 + 64) : (const float *)nullptr,
                       trunk ? (const unsigned *)net->tumask : (const unsigned *)nullptr);
    if (trunk) {
        // sum of DZ3 over the unaffected conv3 pixels: the rank-1 term of conv3's weight gradient (trunk_rank1_kernel); over all pixels:
        // conv3's bias gradient of this chunk, added by trunk_closed3_kernel, which also needs it
        RJob two[2] = {};
        two[0].kind = RJ_NARROW; two[0].blocks = (64 + kNarrowCols - 1) / kNarrowCols; two[0].i0 = nenv < hg3 ? nenv : hg3; two[0].i1 = 0; two[0].n = 64;
        two[0].p0 = net->tslab + 2048 * 64; two[0].d0 = net->tsums + 128;
        two[1] = two[0]; two[1].p0 = net->slab1b; two[1].d0 = net->tsums + 192;
        rb_launch(net, two, 2);
        // the pixels outside the union mask, which agent_dz3 did not see
        hipLaunchKernelGGL(trunk_upix_kernel, dim3(49), dim3(256), 0, st, P + ConvOffsets::d1w, (const float *)net->tug, (const unsigned *)net->tumask,
                           net->tuspix);
        hipLaunchKernelGGL(trunk_uadd_kernel, dim3(1), dim3(64), 0, st, (const float *)net->tuspix, (const float *)(net->tbgz3 + 64), net->tsums);
    } else {
        RJob j{};      // conv3's bias gradient
        j.kind = RJ_NARROW; j.blocks = (64 + kNarrowCols - 1) / kNarrowCols; j.i0 = nenv < hg3 ? nenv : hg3; j.i1 = 1; j.n = 64; j.p0 = net->slab1b; j.d0 = Gr + ConvOffsets::c3b;
        rq_push(net, RD_C3B, j);
    }
    // conv3's data gradient on the shared a2 (net_shared.inc): per-env T3 of the agent-summed dz3 under the shared
    // mask, T3(dz3_a) at the <= 9 touched pixels of every agent, then the exact per-agent mask corrections
    net->prof_tag_cur = PT_ENV_DGRAD;
    if (trunk) {      // at the affected conv2 rows only: the others enter the conv2-level gradients as a sum (trunk_closed3_kernel)
        float *cs4 = slabb_take(net, ((size_t)nenv * 81 / 128 + 2) * 4 * 64);
        if (!cs4) return paac_fail(net, GRL_E_INVALID, "backward_chunk: column-sum buffer too small");
        rowk_launch<128, 64, 4, 1, false, 1, true>(net, GatherT3Rows{net->dz3sh, net->trowlist, net->trows_n, nenv * 81}, net->w3t, 576, 64,
                                   EpiGradRowsSum{net->dz2, 64, net->a2sh, cs4, net->trowlist, net->trows_n},
                                   2.0 * trunk_live(net, 0, (double)nenv * 81) * 576 * 64);
        hipLaunchKernelGGL(colsum_live_kernel, dim3(kLiveParts), dim3(256), 0, st, (const float *)cs4, (const int *)net->trows_n, 128, 4, 64,
                           net->cfold);
    } else if (nenv % 256 == 0)
        rowk_launch<256, 64, 4, 1, false>(net, GatherT3PM{net->dz3sh, nenv * 81, nenv}, net->w3t, 576, 64,
                                   EpiGradPM{net->dz2, net->a2sh, nenv, 81, 64}, 2.0 * nenv * 441 * 64 * 64);
    else
        rowk_launch<256, 64, 4, 1, false>(net, GatherT3{net->dz3sh, nenv * 81}, net->w3t, 576, 64, EpiGrad{net->dz2, 64, net->a2sh},
                                   2.0 * nenv * 81 * 576 * 64);
    return GRL_OK;
}

// T3(dz3_a) at the <= 9 touched pixels of every agent, then the exact per-agent mask corrections of conv3's data gradient (agent_dz2).
// Queues: RD_C2B (without the trunk skip)
static int bwd_slot_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    net->prof_tag_cur = PT_SLOT_DGRAD;
    hipLaunchKernelGGL(slot_rowdesc_kernel, dim3((n * 9 + 255) / 256), dim3(256), 0, st, net->rowagent, net->ulist, net->org, net->sbase + n,
                       net->sperm, n * 9, net->rowdesc);
    {   // 128 x 64 tiles on four waves with one accumulator set (four waves per SIMD): 78.5 -> 71 us per chunk against the 256 x 64
        // four-wave form (interior 187 -> 180); the 256 x 64 eight-wave form measured 87.5 (222)
        SlotGatherT3P g3{net->dz3p, net->rowdesc, n * 9, net->sbase + n, net->sperm, net->patch_skip ? net->stmask : nullptr, nullptr};
        GemmTimer t(net, 2.0 * slot_rows_for_flops(net, n) * 576 * 64 * net->sfrac);
        // (round 5: a contiguous range of row tiles per XCD, as the conv3 patch gather has it, changed nothing of this launch's L2-miss
        // fetch -- 0.82 GB with every agent in the interior either way -- and cost 178 -> 191 us there, 71 -> 89 on the rim: not used)
        launch_rowk<128, 64, 4, 1, SlotGatherT3P, EpiPermStore, true, true, 1, true>(net, dim3(1, (n * 9 + 127) / 128), st, g3, net->w3t, 576, 64,
                                                                                     EpiPermStore{net->gsl, net->sperm, 64});
    }
    static const int hg2 = resident_grid((const void *)agent_dz2_kernel, 2048);
    maybe_evict(net);
    float *slab1b_dz2 = net->slab1b + (size_t)2048 * 64;
    hipLaunchKernelGGL(agent_dz2_kernel, dim3(nenv < hg2 ? nenv : hg2), dim3(256), 0, st, net->gsl, net->m2s, net->a2sh, net->ulist,
                       net->sbase, nenv, net->dz2, net->dza, slab1b_dz2, trunk ? (const unsigned *)net->tamask : (const unsigned *)nullptr,
                       trunk ? 1 : 0);
    if (trunk) {      // tsums[0..63]: dz2 summed over all rows (conv2's bias gradient of the chunk), [64..127]: over the unaffected rows
        hipLaunchKernelGGL(slab_reduce_narrow_kernel, dim3((64 + kNarrowCols - 1) / kNarrowCols), dim3(256), 0, st, slab1b_dz2, nenv < hg2 ? nenv : hg2, 64, net->tsums, 0);
        hipLaunchKernelGGL(trunk_closed3_kernel, dim3(1), dim3(256), 0, st, P + ConvOffsets::c3w, (const float *)(net->tbgz + 64),
                           (const float *)net->cfold, net->tsums, Gr + ConvOffsets::c3b);
    } else {
        RJob j{};      // conv2's bias gradient
        j.kind = RJ_NARROW; j.blocks = (64 + kNarrowCols - 1) / kNarrowCols; j.i0 = nenv < hg2 ? nenv : hg2; j.i1 = 1; j.n = 64; j.p0 = slab1b_dz2; j.d0 = Gr + ConvOffsets::c2b;
        rq_push(net, RD_C2B, j);
    }
    return GRL_OK;
}

// conv2 / conv1 gradients once per ENV on the agent-summed dz2.  Queues: RD_C1B
static int bwd_conv2_dgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    net->prof_tag_cur = PT_ENV_DGRAD;
    // dS = relu'(S) . T2(DZ2): the mask comes from the stored pre-activation, the column sums (conv1's bias gradient up to
    // the per-agent corrections agent_ds_kernel adds) from the epilogue
    float *cs5 = slabb_take(net, ((size_t)nenv * 100 / 128 + 2) * kW128M * 128);
    if (!cs5) return paac_fail(net, GRL_E_INVALID, "backward_chunk: column-sum buffer too small");
    if (trunk) {      // at the touched 2x2 pixel blocks only: nobody reads dS anywhere else (net_shared.inc, trunk_mark_kernel)
        rowk_launch<128, 128, 2, 2, false>(net, GatherT2Rows{net->dz2, net->tblklist, net->trows_n + 1, nenv * 100}, net->w2t, 256, 128,
                                    EpiGradStride2Rows{net->gt, net->sraw, cs5, P + ConvOffsets::c1b, net->tblklist, net->trows_n + 1},
                                    2.0 * trunk_live(net, 1, (double)nenv * 100) * 256 * 128);
        hipLaunchKernelGGL(fold_class_sums_kernel, dim3(kFoldParts), dim3(256), 0, st, cs5, (nenv * 100 + 127) / 128 * 2, net->cfold,
                           (const int *)(net->trows_n + 1));
    } else {
        rowk_launch<128, 128, 2, 2, false>(net, GatherT2{net->dz2, nenv * 100}, net->w2t, 256, 128,
                                    EpiGradStride2<true, true>{net->gt, net->sraw, cs5}, 2.0 * nenv * 100 * 256 * 128);
        hipLaunchKernelGGL(fold_class_sums_kernel, dim3(kFoldParts), dim3(256), 0, st, cs5, (nenv * 100 + 127) / 128 * 2, net->cfold,
                           (const int *)nullptr);
    }
    {   // cfold is not written again in this chunk: the final fold into conv1's bias gradient is queued
        RJob j{};
        j.kind = RJ_FOLDFINAL; j.blocks = 1; j.p0 = net->cfold; j.d0 = Gr + ConvOffsets::c1b;
        rq_push(net, RD_C1B, j);
    }
    return GRL_OK;
}

// ---- weight gradients
// the dense stack's, common to both trunks.  Queues: RD_V2W, RD_V1W, RD_P1W, RD_D2W
static int bwd_dense_wgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    int rc;
    if ((rc = tn_launch<128, 128, 2, 2>(net, RD_V2W, DenseRows{net->v1, n, 512, 512}, 512, net->gv2, 256, Gr + net->ho.v2w, 1, 0.0, 0, net->tn_wgs_dense))) return rc;
    if ((rc = tn_launch<128, 128, 2, 2>(net, RD_V1W, DenseRows{net->d2, n, 256, 256}, 256, net->gv1, 512, Gr + net->ho.v1w, 1, 0.0, 0, net->tn_wgs_dense))) return rc;
    if ((rc = tn_launch<128, 128, 2, 2>(net, RD_P1W, DenseRows{net->d2, n, 256, 256}, 256, net->gp1, 512, Gr + ConvOffsets::p1w, 1, 0.0, 0, net->tn_wgs_dense))) return rc;
    if ((rc = tn_launch<128, 128, 2, 2>(net, RD_D2W, DenseRows{net->d1, n, 512, 512}, 512, net->gd2, 256, Gr + ConvOffsets::d2w, 1, 0.0, 0, net->tn_wgs_dense))) return rc;
    return GRL_OK;
}

// dW_dense1 = a3sh^T (sum_a gd1_a) per env + per-group d3^T gd1 on the patch rows.  Queues: RD_D1W twice (per env, then the patch slices)
static int bwd_dense1_wgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    int rc;
    net->prof_tag_cur = PT_ENV_WGRAD;
    if (trunk) {      // rows of the union mask's pixels; the others are a3bg (x) G (slab_reduce_umask_kernel)
        constexpr int I = 3136, J = 512;
        int chunks, mc;
        float *slab = slab_plan_take(net, net->tn_wgs, (I / 64) * (J / 128), 0, nenv, (size_t)I * J, "dense1 per-env weight gradient: slab too small", &chunks, &mc);
        if (!slab) return GRL_E_INVALID;
        {
            GemmTimer t(net, 2.0 * nenv * 64.0 * trunk_union_pixels(net) * J);
            launch_tn<64, 128, 2, 2, DenseRowsIU>(net, dim3(I / 64, J / 128, chunks), st, DenseRowsIU{{net->a3sh, nenv, 3136, 3136}, net->tumask},
                                                  net->gd1sh, J, mc, slab);
        }
        RJob j{};
        j.kind = RJ_UMASK; j.blocks = (int)(((long)I * J + 255) / 256); j.i0 = chunks; j.n = (long)I * J; j.p0 = slab; j.p1 = net->tumask;
        j.p2 = net->tbgz3 + 64; j.p3 = net->tug; j.d0 = Gr + ConvOffsets::d1w;
        rq_push(net, RD_D1W, j);
    } else if ((rc = tn_launch<64, 128, 2, 2>(net, RD_D1W, DenseRows{net->a3sh, nenv, 3136, 3136}, 3136, net->gd1sh, 512, Gr + ConvOffsets::d1w))) return rc;
    {
        float *pslab = slab_take(net, (size_t)net->pslices * 1600 * 512);
        if (!pslab) return paac_fail(net, GRL_E_INVALID, "backward_chunk: slab too small for the patch slices");
        PatchRows g{net->d3, net->perm, net->tilegroup, net->ptiles * 256, 1600, 1600, 0, net->sbeg, net->send, net->patch_skip ? net->tmask : nullptr,
                    net->patch_skip ? net->zmask : nullptr};
        {
            net->prof_tag_cur = PT_PATCH_WGRAD;
            GemmTimer t(net, 2.0 * n * 1600 * 512 * net->pfrac[2]);
            if (net->pwgrad_pair) {      // two live pixels per 128-wide I tile: 13 tiles cover any support
                PatchRowsPair gp{g};
                if (net->pwgrad_xcd == 1)
                    launch_tn<128, 128, 2, 2, PatchRowsPair, 1>(net, dim3(13, 512 / 128, net->pslices), st, gp, net->gd1, 512, 0, pslab);
                else
                    launch_tn<128, 128, 2, 2, PatchRowsPair, 0>(net, dim3(13, 512 / 128, net->pslices), st, gp, net->gd1, 512, 0, pslab);
            } else if (net->pwgrad_xcd == 1)
                launch_tn<64, 128, 2, 2, PatchRows, 1>(net, dim3(1600 / 64, 512 / 128, net->pslices), st, g, net->gd1, 512, 0, pslab);
            else if (net->pwgrad_xcd == 2)
                launch_tn<64, 128, 2, 2, PatchRows, 2>(net, dim3(1600 / 64, 512 / 128, net->pslices), st, g, net->gd1, 512, 0, pslab);
            else
                launch_tn<64, 128, 2, 2, PatchRows, 0>(net, dim3(1600 / 64, 512 / 128, net->pslices), st, g, net->gd1, 512, 0, pslab);
        }
        RJob j{};
        j.kind = RJ_PATCH; j.blocks = 3136 * 128 / 256; j.i0 = net->pslices; j.p0 = pslab; j.p1 = net->sgrp; j.p2 = net->patch_skip ? net->zmask : nullptr;
        j.d0 = Gr + ConvOffsets::d1w;
        rq_push(net, RD_D1W, j);
    }
    return GRL_OK;
}

// dW3 = patches(a2sh)^T DZ3 + sum over (agent, slot) of (a2_a - a2sh)[u] (x) dz3_a[u - tap].  Queues: RD_C3W (with the trunk skip: the
// affected rows, then the rank-1 term), then RD_C3W again for the slot correction
static int bwd_conv3_wgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    int rc;
    net->prof_tag_cur = PT_ENV_WGRAD;
    if (trunk) {      // the affected conv3 rows + the rank-1 term of the rest (see conv2's below)
        constexpr int I = 576, J = 64;
        int chunks;      // rows 0: they are dealt to the row ranges on the device
        float *slab = slab_plan_take(net, net->tn_wgs, (I / 64) * (J / 64), 0, 0, (size_t)I * J, "conv3 weight gradient: slab too small", &chunks);
        if (!slab) return GRL_E_INVALID;
        GatherConv3Rows ag{net->a2sh, net->tc3list, net->trows_n + 2, net->tbgimg3, nenv * 49, chunks};
        {
            GemmTimer t(net, 2.0 * trunk_live(net, 2, (double)nenv * 49) * I * J);
            launch_tn<64, 64, 2, 2, GatherConv3Rows>(net, dim3(I / 64, J / 64, chunks), st, ag, net->dz3sh, J, 0, slab);
        }
        RJob j{};
        j.kind = RJ_SLAB; j.blocks = (I * J + 255) / 256; j.i0 = chunks; j.i1 = 1; j.n = (long)I * J; j.p0 = slab; j.d0 = Gr + ConvOffsets::c3w;
        rq_push(net, RD_C3W, j);
        RJob r{};      // the rank-1 term of the unaffected rows (trunk_rank1_kernel)
        r.kind = RJ_RANK1; r.blocks = I * J / 256; r.i0 = 63; r.p0 = net->tbgz + 64; r.p1 = net->tsums + 128; r.d0 = Gr + ConvOffsets::c3w;
        rq_push(net, RD_C3W, r);
    } else if ((rc = tn_launch<64, 64, 2, 2>(net, RD_C3W, GatherConv3{net->a2sh, nenv * 49}, 576, net->dz3sh, 64, Gr + ConvOffsets::c3w))) return rc;
    net->prof_tag_cur = PT_SLOT_WGRAD;
    // >= 684 row ranges: the gather loop is bound by the latency of its loads, one K-tile in flight per workgroup at three
    // workgroups per CU, so its time falls with the workgroups in flight (round 5, rim / interior us per chunk: 228 ranges 175 / 235,
    // 456: 124 / 237, 684: 89 / 237, 912: 107 / 241)
    if ((rc = slot_wgrad_launch(net, n, Gr + ConvOffsets::c3w, slot_rows_for_flops(net, n), 684))) return rc;
    return GRL_OK;
}

// conv2's weight gradient once per env.  Queues: RD_C2W (with the trunk skip: the affected rows, then RD_C2W, RD_C1B, RD_C2B for
// trunk_closed_kernel's three parts)
static int bwd_conv2_wgrad(const BwdCtx &c) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    int rc;
    net->prof_tag_cur = PT_ENV_WGRAD;
    if (trunk) {
        // the affected rows of every env (trunk_index), dealt evenly to the row ranges on the device; the rest of the rows are one
        // constant patch: trunk_closed_kernel adds their rank-1 term (and the two closed-form bias parts)
        constexpr int I = 512, J = 64;
        int chunks;      // rows 0: dealt on the device
        float *slab = slab_plan_take(net, net->tn_wgs, (I / 128) * (J / 64), 0, 0, (size_t)I * J, "conv2 weight gradient: slab too small", &chunks);
        if (!slab) return GRL_E_INVALID;
        GatherConv2ReluRows ag{net->sraw, net->trowlist, net->trows_n, net->tbgimg, nenv * 81, chunks};
        {
            GemmTimer t(net, 2.0 * trunk_live(net, 0, (double)nenv * 81) * I * J);
            launch_tn<128, 64, 2, 2, GatherConv2ReluRows>(net, dim3(I / 128, J / 64, chunks), st, ag, net->dz2, J, 0, slab);
        }
        RJob j{};
        j.kind = RJ_SLAB; j.blocks = (I * J + 255) / 256; j.i0 = chunks; j.i1 = 1; j.n = (long)I * J; j.p0 = slab; j.d0 = Gr + ConvOffsets::c2w;
        rq_push(net, RD_C2W, j);
        // trunk_closed_kernel's three parts: the rank-1 background term of dW2, conv1's closed-form bias part, conv2's bias gradient
        RJob w{};
        w.kind = RJ_CLOSED_W; w.blocks = 128; w.p0 = P + ConvOffsets::c1b; w.p1 = net->tsums + 64; w.d0 = Gr + ConvOffsets::c2w;
        rq_push(net, RD_C2W, w);
        RJob b1{};
        b1.kind = RJ_CLOSED_B1; b1.blocks = 1; b1.p0 = P + ConvOffsets::c1b; b1.p1 = P + ConvOffsets::c2w; b1.p2 = net->tsums; b1.d0 = Gr + ConvOffsets::c1b;
        rq_push(net, RD_C1B, b1);
        RJob b2{};
        b2.kind = RJ_CLOSED_B2; b2.blocks = 1; b2.p0 = net->tsums; b2.d0 = Gr + ConvOffsets::c2b;
        rq_push(net, RD_C2B, b2);
    } else if ((rc = tn_launch<128, 64, 2, 2>(net, RD_C2W, GatherConv2Relu{net->sraw, nenv * 81}, 512, net->dz2, 64, Gr + ConvOffsets::c2w))) return rc;
    return GRL_OK;
}

// the per-agent trunk's weight and bias gradients of dense1 and the convolutions.  Queues: RD_D1W, RD_C3W, RD_C2W, RD_C3B, RD_C2B, RD_C1B;
// conv1's weight gradient is reduced at once
static int bwd_per_agent_wgrad(const BwdCtx &c, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    int rc;
    if ((rc = tn_launch<64, 128, 2, 2>(net, RD_D1W, DenseRows{net->a3, n, 3136, 3136}, 3136, net->gd1, 512, Gr + ConvOffsets::d1w))) return rc;
    if ((rc = tn_launch<64, 64, 2, 2>(net, RD_C3W, GatherConv3{net->a2, n * 49}, 576, net->ga3, 64, Gr + ConvOffsets::c3w))) return rc;
    if ((rc = tn_launch<128, 64, 2, 2>(net, RD_C2W, GatherConv2{net->a1, n * 81}, 512, net->ga2, 64, Gr + ConvOffsets::c2w))) return rc;
    // ---- bias gradients
    // (the bias gradients of v2 and pol1 -- column sums of gv2 / gp1 -- come out of heads_backward_kernel's slab row)
    if ((rc = colsum_launch(net, RD_C3B, net->ga3, n * 49, 64, Gr + ConvOffsets::c3b))) return rc;      // shared: out of agent_dz3_kernel
    if ((rc = colsum_launch(net, RD_C2B, net->ga2, n * 81, 64, Gr + ConvOffsets::c2b))) return rc;
    if ((rc = colsum_launch(net, RD_C1B, net->ga1, n * 400, 32, Gr + ConvOffsets::c1b))) return rc;
    // ---- conv1 weights (sparse)
    const int blocks = nenv < 512 ? nenv : 512;
    hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(blocks), dim3(256), 0, st, lb, ab, pos, net->ga1, nenv, net->h->cfg.grid_size,
                       net->slab64, (const float *)nullptr);
    hipLaunchKernelGGL(slab64_reduce_kernel, dim3(6144 / 256), dim3(256), 0, st, net->slab64, blocks, 6144, Gr + ConvOffsets::c1w);
    return GRL_OK;
}

// per-agent corrections: dW2 (+=), one-hot taps of dW1 (+=), and gt: T2(DZ2) -> dS in place; then conv1's weight gradient.
// Queues: RD_C2W, RD_C1W_HOT, RD_C1B, RD_C1W_CNT
static int bwd_class_corr_conv1(const BwdCtx &c, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos) {
    const auto [net, st, P, Gr, n, nenv, trunk] = c;
    static const int hgs = resident_grid((const void *)agent_ds_kernel, 2048);
    const int dblocks = nenv < hgs ? nenv : hgs, npad = net->npad;
    maybe_evict(net);
    const int t2rows = (n + 127) / 128 * 128;      // rows of the class GEMMs' last tile exist as (invalid) descriptors
    hipLaunchKernelGGL(gather_t2_kernel, dim3((t2rows + kT2Agents - 1) / kT2Agents), dim3(256), 0, st, net->sraw, pos, net->ulist, net->sbase,
                       P + ConvOffsets::c1w, n, npad, t2rows, net->t2desc, net->dl2);
    net->prof_tag_cur = PT_CLASS_CORR;
    {   // the four parity classes in one launch each (they are launch-latency bound one by one): T2 rows and dW2
        const int cpc = 64;                                        // row ranges per class: 4 x 64 x 8 tiles = 2 048 workgroups
        const int mc = ((n + cpc - 1) / cpc + 31) / 32 * 32;
        T2SlotGather g{net->dza, net->t2desc, 4 * npad, npad, n, 32, cpc};
        {
            GemmTimer t(net, 4 * 2.0 * n * 256 * 32);
            launch_rowk<128, 32, 4, 1, T2SlotGather, EpiStore>(net, dim3(1, 4 * npad / 128), st, g, net->w2t, 256, 32, EpiStore{net->tt2, 32});
        }
        float *cslab = slab_take(net, (size_t)4 * cpc * 8192);
        if (!cslab) return paac_fail(net, GRL_E_INVALID, "class corrections: slab too small");
        {
            GemmTimer t(net, 4 * 2.0 * n * 256 * 32);
            launch_tn<64, 32, 4, 1, T2SlotGather>(net, dim3(256 / 64, 1, 4 * cpc), st, g, net->dl2, 32, mc, cslab);      // one tap per I tile: its validity is per row
        }
        RJob j{};      // the grouped slab sum and conv2_corr_add's re-indexing into dW2 in one queued job
        j.kind = RJ_GROUPS_C2; j.blocks = 4 * 8192 / 256; j.i0 = cpc; j.p0 = cslab; j.d0 = Gr + ConvOffsets::c2w;
        rq_push(net, RD_C2W, j);
    }
    float *slab1h = net->slab1h, *slab1b_ds = net->slab1b + (size_t)2 * 2048 * 64;
    // (both forms on the parent kernels' grids: the workgroup an env falls to decides the order of the sums)
    if (net->obs_index)
        hipLaunchKernelGGL(agent_ds_indexed_kernel, dim3(dblocks), dim3(256), 0, st, net->sraw, (const unsigned *)net->obsrec, net->tt2, npad, net->gt,
                           P + ConvOffsets::c1w, nenv, slab1h, slab1b_ds);
    else
        hipLaunchKernelGGL(agent_ds_kernel, dim3(dblocks), dim3(256), 0, st, net->sraw, pos, net->tt2, npad, net->gt, P + ConvOffsets::c1w,
                           nenv, slab1h, slab1b_ds);
    {
        RJob j{};
        j.kind = RJ_ONEHOT; j.blocks = 2048 / 16; j.i0 = dblocks; j.p0 = slab1h; j.d0 = Gr + ConvOffsets::c1w;
        rq_push(net, RD_C1W_HOT, j);
        // conv1's bias gradient: the base part came out of the T2 GEMM's epilogue, agent_ds_kernel adds the sums of its corrections
        RJob b{};
        b.kind = RJ_NARROW; b.blocks = (32 + kNarrowCols - 1) / kNarrowCols; b.i0 = dblocks; b.i1 = 1; b.n = 32; b.p0 = slab1b_ds; b.d0 = Gr + ConvOffsets::c1b;
        rq_push(net, RD_C1B, b);
    }
    // one resident wave of workgroups at six waves per SIMD (80 registers, 20 bytes of scratch): the kernel is a per-env chain of
    // dependent steps, so its time falls with the workgroups in flight -- 768: 175 us per 8 192-env chunk, 1 024: 143, 1 280: 121-125, 1 536:
    // 116 (round 4; the 32 KB LDS accumulators that had made 1 280 slower than 1 024 in round 3 are registers since then)
    static const int hgw = resident_grid((const void *)conv1_wgrad_shared_kernel, 1536);
    // conv1_wgrad_indexed_kernel runs on THIS grid too, taken from the other kernel's occupancy on purpose: the workgroup an env falls to
    // decides the order of the slab sums, and GRL_OBS_INDEX=off / on are held bit for bit against each other (tests/test_gpu_obs_index.py).
    // Both kernels are bound to six waves per SIMD, so the grid is one resident wave of workgroups for either.  Without that test the
    // barrier-free kernel could take fewer, wider workgroups (fewer 32 KB slabs to write and reduce): not measured.
    const int wblocks = nenv < hgw ? nenv : hgw;
    if (net->obs_index)
        hipLaunchKernelGGL(conv1_wgrad_indexed_kernel, dim3(wblocks), dim3(256), 0, st, (const unsigned *)net->obsrec, (const float *)net->gt, nenv,
                           net->slab64);
    else
        hipLaunchKernelGGL(conv1_wgrad_shared_kernel, dim3(wblocks), dim3(256), 0, st, lb, ab, (const float *)net->gt, nenv,
                           net->h->cfg.grid_size, net->slab64);
    RJob j{};
    j.kind = RJ_SLAB64; j.blocks = 4096 / 16; j.i0 = wblocks; j.p0 = net->slab64; j.d0 = Gr + ConvOffsets::c1w;
    rq_push(net, RD_C1W_CNT, j);
    return GRL_OK;
}

// The stages above in the one order that keeps the gradient's bits.  Two things here are order, not style:
//  - rq_push per destination (RD_*): the k-th job queued for a destination runs in phase k of rq_flush, so the order of the pushes is the
//    order of the float sums into that gradient (RD_D1W: per env, then the patch slices; RD_C3W, RD_C2W, RD_C1B, RD_C2B likewise);
//  - slab_take / slabb_take, in order and size: a request that does not fit flushes the queue first, and the jobs queued by then are
//    summed into the gradient ahead of every later one.  A stage that moves, or a slab that changes size, moves that point.
static int backward_chunk_body(grl_net *net, const TrainBufs &tb, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, int nenv,
                               const float *actions, const float *adv, const float *y, float inv_total, long slot,
                               const float *pmu, const float *psg, const float *pval) {
    const BwdCtx c{net, net->h->stream, net->params, net->grads, nenv * 10, nenv, net->trunk_skip && net->expand2_gemm};
    const bool shared = net->shared_trunk;
    bind_activations(net, slot);
    // pmu / psg / pval: the heads' outputs the ROLLOUT computed for these samples (same parameters, same kernel: the same bits); with
    // the dense stack resident too, the gradient step does not evaluate the heads again (49 us and 252 MB per chunk)
    const bool have_heads = slot >= 0 && pmu && psg && pval;
    int rc = forward_chunk(net, lb, ab, pos, nenv, tb.cmu, tb.csigma, tb.cvs, slot >= 0, have_heads);
    if (rc) return rc;
    // the observation's index record for conv1's backward helpers at the end of this pass: a small kernel, enqueued here so that it runs
    // behind the GEMMs in between (lane scratch like the trunk lists: rebuilt per pass, not kept with the rollout)
    if (shared && net->obs_index && (rc = obs_index(net, lb, ab, pos, nenv, net->obsrec, c.st, 2))) return rc;
    if ((rc = bwd_heads(c, tb, have_heads ? pmu : tb.cmu, have_heads ? psg : tb.csigma, have_heads ? pval : tb.cvs, actions, adv, y, inv_total))) return rc;
    net->prof_tag_cur = shared ? PT_DENSE_DGRAD : PT_PER_AGENT;
    if ((rc = bwd_dense_dgrad(c))) return rc;
    if (shared) {
        if ((rc = bwd_dense1_dgrad(c)) || (rc = bwd_conv3_dgrad(c)) || (rc = bwd_slot_dgrad(c)) || (rc = bwd_conv2_dgrad(c))) return rc;
    } else if ((rc = bwd_per_agent_dgrad(c))) return rc;
    PAAC_HIP(net, hipGetLastError());
    net->prof_tag_cur = shared ? PT_DENSE_WGRAD : PT_PER_AGENT;
    if ((rc = bwd_dense_wgrad(c))) return rc;
    if (shared) {
        if ((rc = bwd_dense1_wgrad(c)) || (rc = bwd_conv3_wgrad(c)) || (rc = bwd_conv2_wgrad(c)) || (rc = bwd_class_corr_conv1(c, lb, ab, pos))) return rc;
    } else if ((rc = bwd_per_agent_wgrad(c, lb, ab, pos))) return rc;
    PAAC_HIP(net, hipGetLastError());
    // the chunk's queued folds into the lane's gradient accumulator: one launch per phase (net_reduce.inc)
    return rq_flush(net);
}

// prepares every active lane (buffers, zeroed gradient accumulator and loss sums); lane 0 is current afterwards.  It makes lanes
// current itself (no fork yet): its callers hold a LanePass from before the call
static int train_begin(grl_net *net, TrainBufs *tb) {
    static_assert(sizeof(double) == 8, "");
    const size_t c = net->chunk;
    const int nl = lanes_active(net);
    hipStream_t main_st = net->lane_stream[0];
    rq_reset(net);      // a pass starts with nothing queued (a failed chunk of an earlier pass cleans up after itself as well)
    for (int k = nl - 1; k >= 0; --k) {      // ends with lane 0 current
        use_lane(net, k);
        int rc = ensure_train_bufs(net);
        if (rc) return rc;
        float *base = net->ro_mu;
        const size_t A = net->ho.A, dz = net->ho.dz;
        tb[k].cmu = base; tb[k].csigma = base + c * A; tb[k].cvs = base + c * 2 * A; tb[k].dzh = tb[k].cvs + c; tb[k].cact = tb[k].dzh + c * dz;
        tb[k].cadv = tb[k].cact + c * A; tb[k].cy = tb[k].cadv + c;
        tb[k].stats64 = net->slab64 + kSlab64Doubles;      // chunk-independent scalars live at the tail of slab64's allocation
        tb[k].partial = tb[k].stats64 + 8;
        PAAC_HIP(net, hipMemsetAsync(net->grads, 0, net->ho.total * 4, main_st));
        PAAC_HIP(net, hipMemsetAsync(tb[k].stats64, 0, 8 * sizeof(double), main_st));
    }
    hipLaunchKernelGGL(transpose_conv_weights_kernel, dim3((576 * 64 + 255) / 256), dim3(256), 0, main_st,
                       net->params + ConvOffsets::c2w, net->params + ConvOffsets::c3w, net->w2t, net->w3t);
    PAAC_HIP(net, hipMemsetAsync(net->stats + kLossBoundAt, 0, sizeof(float), main_st));
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// rows [0, n) of (mu, sigma, vs, actions, adv, y) enter the bound of this pass's head gradients (main stream, lane 0)
static int train_bound_rows(grl_net *net, const float *mu, const float *sigma, const float *vs, const float *actions, const float *adv,
                            const float *y, long n) {
    GRL_HEADS_DISPATCH(net->ho.A, hipLaunchKernelGGL(head_bound_kernel<kA>, dim3((unsigned)std::min<long>((n + 255) / 256, 2048)), dim3(256), 0, net->lane_stream[0], mu,
                                                     sigma, vs, actions, adv, y, n, net->cfg.scale, net->cfg.entropy_beta,
                                                     reinterpret_cast<unsigned *>(net->stats + kLossBoundAt)));
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// fixes the loss scale of the pass from the bound collected so far, then forks the lanes off the main stream
static int train_scale_and_fork(grl_net *net, float inv_total) {
    hipLaunchKernelGGL(loss_scale_kernel, dim3(1), dim3(64), 0, net->lane_stream[0], reinterpret_cast<const unsigned *>(net->stats + kLossBoundAt),
                       inv_total, net->loss_scale_on, net->stats + kLossScaleAt);
    PAAC_HIP(net, hipGetLastError());
    return lanes_fork(net);
}

// lane k's gradient accumulator and loss sums folded into lane 0's (one launch per lane, k = 1, 2, ...: a fixed order, deterministic)
__global__ void lane_fold_kernel(float *__restrict__ g0, const float *__restrict__ g1, long n, double *__restrict__ s0,
                                 const double *__restrict__ s1) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g0[i] += g1[i];
    if (i < 8) s0[i] += s1[i];
}

// joins the lanes, folds their gradient accumulators and loss sums into lane 0's (fixed order) and removes the loss scale
static int train_fold(LanePass<grl_net> &pass, const TrainBufs *tbs) {
    grl_net *net = pass.net;
    const int nl = lanes_active(net);
    int jrc = pass.finish();
    if (jrc) return jrc;
    for (int k = 1; k < nl; ++k)
        hipLaunchKernelGGL(lane_fold_kernel, dim3((unsigned)((net->ho.total + 255) / 256)), dim3(256), 0, net->h->stream, net->grads,
                           net->lanes[k].grads, (long)net->ho.total, tbs[0].stats64, tbs[k].stats64);
    hipLaunchKernelGGL(unscale_grads_kernel, dim3((unsigned)((net->ho.total + 255) / 256)), dim3(256), 0, net->h->stream, net->grads,
                       (long)net->ho.total, (const float *)(net->stats + kLossScaleAt));
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// global norm of grad_scale * grads, clip factor, loss statistics; then (apply_update) Adam on lane 0's gradient
static int train_apply(grl_net *net, float inv_total, float lr, int apply_update, float grad_scale, float *stats_host) {
    hipStream_t st = net->h->stream;
    double *stats64 = net->slab64 + kSlab64Doubles, *partial = stats64 + 8;      // lane 0 (current after train_fold)
    const int nparts = 1024;
    hipLaunchKernelGGL(paac_sumsq_kernel<>, dim3(nparts), dim3(256), 0, st, net->grads, (long)net->ho.total, partial);
    hipLaunchKernelGGL(finalize_stats_kernel, dim3(1), dim3(64), 0, st, partial, nparts, stats64, inv_total, net->cfg.clip_norm,
                       grad_scale, net->stats);
    int *latch = reinterpret_cast<int *>(net->stats + kRangeLatchAt);
    if (apply_update) {
        net->adam_t += 1;
        net->param_version += 1;
        const float lr_t = adam_lr_t(lr, net->adam_t);
        hipLaunchKernelGGL(paac_adam_kernel<>, dim3((unsigned)((net->ho.total + 255) / 256)), dim3(256), 0, st, net->params, net->grads,
                           net->adam_m, net->adam_v, (long)net->ho.total, net->stats, lr_t, (const int *)range_flag_ptr(net));
        // the gradient pass's flag is settled HERE: what refresh_transposes' background GEMMs raise belongs to the next pass
        hipLaunchKernelGGL(range_latch_kernel, dim3(1), dim3(1), 0, st, range_flag_ptr(net), latch);
        refresh_transposes(net);
    }
    PAAC_HIP(net, hipGetLastError());
    const double t_sync0 = host_now_ms();
    PAAC_HIP(net, hipStreamSynchronize(st));
    if (net->ht_train_t0 > 0.0) {      // grl_net_host_times: the gradient step's enqueue work ends where its first blocking call begins
        const double t_sync1 = host_now_ms();
        net->ht_train_enq_ms += t_sync0 - net->ht_train_t0;
        net->ht_train_wait_ms += t_sync1 - t_sync0;
        net->ht_updates += 1;
        net->ht_train_t0 = 0.0;
    }
    paac_allreduce_account(net);
    if (apply_update) {
        int lflag = 0;
        PAAC_HIP(net, hipMemcpy(&lflag, latch, sizeof(int), hipMemcpyDeviceToHost));
        if (lflag) {      // rollout + backward of this update: paac_adam_kernel skipped the update on the device, parameters and moments are intact
            net->range_bits_last = lflag;
            net->adam_t -= 1;      // (param_version stays advanced: the retry recomputes its forward passes in the form it runs in)
            // (the background pass ran on the unchanged parameters: whatever it raised is that of the rows already in use)
            PAAC_HIP(net, hipMemset(range_flag_ptr(net), 0, sizeof(int)));
            return paac_fail(net, GRL_E_RANGE, "gradient pass: an activation or gradient exceeded 65504, the range of the fp16 matrix-pipe GEMMs "
                                           "(include/goldsrl_net.h, Arithmetic); the results of this call are not valid");
        }
        // only the background pass on the UPDATED parameters left the range: the update stands (it was computed and applied from valid
        // operands); the net moves to the fp32 form for what follows, which recomputes the background rows.  Every rank holds the same
        // parameters, so every rank takes this branch together.  With the fallback off the flag stays up and the next call fails.
        int bflag = 0;
        PAAC_HIP(net, hipMemcpy(&bflag, range_flag_ptr(net), sizeof(int), hipMemcpyDeviceToHost));
        net->range_bits_last = 0;
        if (bflag && net->range_fallback_on) {
            PAAC_HIP(net, hipMemset(range_flag_ptr(net), 0, sizeof(int)));
            if (!range_fall_back(net)) (void)trunk_background(net);
            PAAC_HIP(net, hipStreamSynchronize(st));
        }
        else if (int rrc = range_maybe_return(net)) return rrc;      // an update on the fp32 form ended cleanly: one step on the way back
    } else if (int rrc = range_check(net, "gradient pass")) {
        return rrc;
    }
    return paac_read_stats(net, stats_host);
}

// reduce: 0 = local statistics only (no all-reduce; the caller applies nothing)
static int train_finish(LanePass<grl_net> &pass, const TrainBufs *tbs, float inv_total, float lr, int apply_update, float *stats_host, int reduce = 1) {
    grl_net *net = pass.net;
    int rc = train_fold(pass, tbs);
    if (rc) return rc;
    net->last_inv_total = inv_total;
    float grad_scale = 1.0f;
    // the GEMMs' range words [flag, largest |output| of the fp32 form as float bits: non-negative floats order like their bits] travel
    // with the gradient (max over ranks): a rank whose pass overflowed makes EVERY replica skip the update and fail the call, instead
    // of erroring alone and leaving its peers blocked in the next collective
    if (reduce && (rc = paac_allreduce_grads(net, net->grads, range_flag_ptr(net), &grad_scale))) return rc;
    return train_apply(net, inv_total, lr, apply_update, grad_scale, stats_host);
}

static int ensure_rollout_bufs(grl_net *net, int T) {
    const int E = net->h->E, B = E * 10;
    if (net->ro_lb && net->T >= T) return GRL_OK;
    const size_t TE = (size_t)T * E, TB = (size_t)T * B;
    int rc = GRL_OK;
    auto A = [&](auto **p, size_t cnt) { if (rc == GRL_OK) rc = paac_alloc(net, p, cnt); };
    A(&net->ro_lb, TE * 160); A(&net->ro_ab, TE * 20); A(&net->ro_pos, TE * 20); A(&net->ro_act, TB * 2); A(&net->ro_envact, (size_t)B * 2);
    A(&net->ro_val, TB); A(&net->ro_rew, TB); A(&net->ro_y, TB); A(&net->ro_adv, TB); A(&net->ro_boot, (size_t)B); A(&net->ro_done, TE);
    A(&net->ro_pmu, TB * 2); A(&net->ro_psg, TB * 2);      // the policy the actions were drawn from: the gradient step bounds its head gradients with it (loss scale)
    if (rc) return rc;
    net->T = T; net->B = B;
    // rollout-resident activations when they fit (with headroom for the training workspace and RCCL)
    if (net->keep) { (void)hipFree(net->keep); net->keep = nullptr; net->keep_slots = 0; }
    net->keep_version = -1;
    net->keep_level = 0;
    net->keep_headroom = 0; net->keep_free_seen = 0;
    if (!(net->cfg.reserved & GRL_NET_F_RECOMPUTE_FORWARD)) {
        const size_t ce = net->chunk / 10, nchunks = ((size_t)E + ce - 1) / ce, slots = (size_t)T * nchunks;
        size_t free_b = 0, total_b = 0;
        PAAC_HIP(net, hipMemGetInfo(&free_b, &total_b));
        if (net->keep_free_capped) free_b = std::min(free_b, net->keep_free_cap);      // GRL_NET_KEEP_FREE_MB: the descent below at any size
        const size_t headroom = ((size_t)12 << 30) + (size_t)net->chunk * 160000;   // training buffers: ~105 KB per chunk sample
        net->keep_headroom = headroom; net->keep_free_seen = free_b;
        const int max_level = net->keep_max_level;      // GRL_NET_KEEP_LEVEL, read by grl_net_create
        const bool lists = net->trunk_skip && net->expand2_gemm;      // level 3 binds the trunk's row lists: they exist in the default (list) form only
        for (int level = net->shared_trunk ? std::min(lists ? 3 : 2, std::max(max_level, 1)) : 1; level >= 1 && !net->keep; --level) {
            const size_t bytes = slots * keep_floats_per_slot(net, level) * sizeof(float);
            if (free_b > bytes + headroom && hipMalloc((void **)&net->keep, bytes) == hipSuccess) { net->keep_slots = slots; net->keep_level = level; }
            else { net->keep = nullptr; (void)hipGetLastError(); }
        }
        if (net->keep) {
            // before anything is written there: the pointer walk over the last slot ends where the slot does (the two are written
            // down twice; a slot that ends anywhere else overlaps its neighbour).  The net is left bound to the workspace: what it
            // was bound to may have been a slot of the buffer freed above, and every user binds before it reads.
            const size_t walked = bind_activations(net, (long)slots - 1);
            bind_activations(net, -1);
            if (walked != keep_floats_per_slot(net, net->keep_level) * sizeof(float)) {
                (void)hipFree(net->keep);
                net->keep = nullptr; net->keep_slots = 0; net->keep_level = 0;
                net->T = 0;      // no rollout stored: the next call comes through here again
                return paac_fail(net, GRL_E_INVALID, "ensure_rollout_bufs: bind_activations and keep_floats_per_slot disagree about a resident slot");
            }
        }
    }
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_net_rollout(grl_net *net, int32_t T, int32_t reward_layout) {
    if (!net || T <= 0 || T > 1024 || (reward_layout != 0 && reward_layout != 1)) return paac_fail(net, GRL_E_INVALID, "grl_net_rollout: bad argument");
    const double ht0 = host_now_ms();
    grl_handle *h = net->h;
    if (net->ho.A != 2) return paac_fail(net, GRL_E_INVALID, "grl_net_rollout: SwarmEnv.step takes (10, 2) actions; this net was built with num_actions != 2");
    hipSetDevice(h->cfg.device_id);
    int rc = ensure_rollout_bufs(net, T);
    if (rc) return rc;
    const int E = h->E, B = E * 10, ce = net->chunk / 10, nchunks = (E + ce - 1) / ce;
    net->T = T;
    net->keep_version = net->keep && (size_t)T * nchunks <= net->keep_slots ? net->param_version : -1;
    if (reward_layout == 1) PAAC_HIP(net, hipMemsetAsync(net->ro_rew, 0, (size_t)T * B * 4, h->stream));
    // Envs are independent, so a chunk of envs is its own T-step pipeline: forward -> a = mu + sigma*N(0,1) -> norm clip -> env step /
    // auto-reset / observe -> bookkeeping -> next forward.  Chunk c always runs on lane c % nl (a HIP stream keeps its order), so
    // the lanes never wait for each other inside the rollout: the fp64 VALU-bound env step and the memory-bound helper kernels of
    // one chunk overlap the MFMA GEMMs of the others, and there is ONE join, before the returns.  (A lock-step rollout -- forward
    // of all chunks, join, one env step over the whole batch, per time step -- left the matrix pipe idle during every env step.)
    LanePass pass(net);
    if ((rc = pass.begin())) return rc;
    const int nl = lanes_active(net);
    net->side_now = nchunks == 1;      // one chunk per step: nothing hides the forward's index kernels -- lane 0's side stream takes them
    SideOff side_off{net};
    const unsigned long counter0 = net->act_counter;
    net->act_counter += (unsigned long)T;
    for (int t = 0; t <= T; ++t)
        for (int c = 0; c < nchunks; ++c) {
            const int e0 = c * ce, ne = E - e0 < ce ? E - e0 : ce;
            use_lane(net, c % nl);
            net->last_lane = net->cur_lane;
            hipStream_t st = h->stream;      // the lane's stream
            if (t == T) {      // bootstrap value of the state after the last step (paac.py:351-358)
                bind_activations(net, -1);
                rc = forward_chunk(net, h->sw.lbins + (size_t)e0 * 160, h->sw.abins + (size_t)e0 * 20, h->sw.pos + (size_t)e0 * 20, ne,
                                   net->mu + (size_t)e0 * 20, net->sigma + (size_t)e0 * 20, net->ro_boot + (size_t)e0 * 10);
                if (rc) return rc;
                continue;
            }
            bind_activations(net, net->keep_version >= 0 ? (long)t * nchunks + c : -1);
            rc = forward_chunk(net, h->sw.lbins + (size_t)e0 * 160, h->sw.abins + (size_t)e0 * 20, h->sw.pos + (size_t)e0 * 20, ne,
                               net->ro_pmu + ((size_t)t * B + (size_t)e0 * 10) * 2, net->ro_psg + ((size_t)t * B + (size_t)e0 * 10) * 2,
                               net->ro_val + (size_t)t * B + (size_t)e0 * 10);
            if (rc) return rc;
            // states[t] = shared_states (paac.py:319): the sampling launch also keeps the compact observation the action was chosen from
            // and zeroes the lane's done counter for the step that follows
            ObsRecord rec{reinterpret_cast<const uint32_t *>(h->sw.lbins + (size_t)e0 * 160), reinterpret_cast<const uint32_t *>(h->sw.abins + (size_t)e0 * 20),
                          reinterpret_cast<const uint32_t *>(h->sw.pos + (size_t)e0 * 20),
                          reinterpret_cast<uint32_t *>(net->ro_lb + ((size_t)t * E + e0) * 160), reinterpret_cast<uint32_t *>(net->ro_ab + ((size_t)t * E + e0) * 20),
                          reinterpret_cast<uint32_t *>(net->ro_pos + ((size_t)t * E + e0) * 20), ne, h->done_count + net->cur_lane};
            hipLaunchKernelGGL(sample_actions_kernel, dim3((ne * 10 + 255) / 256), dim3(256), 0, st, net->ro_pmu + (size_t)t * B * 2,
                               net->ro_psg + (size_t)t * B * 2, e0 * 10, ne * 10, h->cfg.seed,
                               (uint32_t)h->cfg.env_id_offset, (uint32_t)(counter0 + (unsigned long)t), net->ro_act + (size_t)t * B * 2, net->ro_envact, rec);
            if ((rc = swarm_launch_step_range(h, net->ro_envact, e0, ne, net->cur_lane, true)) ||
                (rc = episodes_launch_account(h, e0, ne)))      // R6 (paac.py:331-349), when enabled on the handle
                return paac_fail(net, rc, h->err);
            hipLaunchKernelGGL(reward_layout_kernel, dim3((ne * 10 + 255) / 256), dim3(256), 0, st, h->reward, e0, ne, reward_layout,
                               net->ro_rew + (size_t)t * B, (const uint8_t *)h->done, net->ro_done + (size_t)t * E);
        }
    if ((rc = pass.finish())) return rc;
    // n-step returns over all columns (paac.py:360-372)
    if ((rc = launch_returns(h, net->ro_rew, net->ro_val, nullptr, net->ro_boot, T, B, net->cfg.gamma, 1.0f, net->cfg.scale, 0.f, 0.f,
                             net->ro_y, net->ro_adv)))
        return paac_fail(net, rc, h->err);
    hipLaunchKernelGGL(rollout_range_mark_kernel, dim3(1), dim3(1), 0, h->stream, range_flag_ptr(net));
    PAAC_HIP(net, hipGetLastError());
    h->step_in_flight = true;
    net->ht_rollout_ms += host_now_ms() - ht0;
    net->ht_rollouts += 1;
    return GRL_OK;
}

// gradient of the last rollout into lane 0's accumulator (every chunk, all lanes, folded); finish: 0 = stop there (local
// statistics only), 1 = all-reduce + clip + Adam
static int train_rollout_impl(grl_net *net, float lr, float *stats_host, int finish) {
    if (!net || !net->ro_lb || net->T <= 0) return paac_fail(net, GRL_E_STATE, "grl_net_train_rollout: no rollout to train on");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    net->ht_train_t0 = host_now_ms();
    TrainBufs tb[GRL_MAX_LANES];
    LanePass pass(net);
    int rc = train_begin(net, tb);
    if (rc) return rc;
    const int E = h->E, B = E * 10, T = net->T, ce = net->chunk / 10;
    const float inv_total = 1.0f / ((float)T * (float)B);
    const int nchunks = (E + ce - 1) / ce, nl = lanes_active(net);
    // same parameters as during the rollout (paac.py:302-387), so its mu / sigma / values are the gradient step's
    if ((rc = train_bound_rows(net, net->ro_pmu, net->ro_psg, net->ro_val, net->ro_act, net->ro_adv, net->ro_y, (long)T * B)) ||
        (rc = train_scale_and_fork(net, inv_total)))
        return rc;
    const bool resident = net->keep && net->keep_version >= 0 && net->keep_version == net->param_version;
    net->resident_last = resident ? 1 : 0;      // grl_net_keep_info
    long ci = 0;
    for (int t = 0; t < T; ++t)
        for (int e0 = 0; e0 < E; e0 += ce, ++ci) {
            int ne = E - e0 < ce ? E - e0 : ce;
            size_t s0 = (size_t)t * B + (size_t)e0 * 10;
            use_lane(net, (int)(ci % nl));      // independent chunks go round the lanes
            rc = backward_chunk(net, tb[net->cur_lane], net->ro_lb + ((size_t)t * E + e0) * 160, net->ro_ab + ((size_t)t * E + e0) * 20,
                                net->ro_pos + ((size_t)t * E + e0) * 20, ne, net->ro_act + s0 * 2, net->ro_adv + s0, net->ro_y + s0,
                                inv_total, resident ? (long)t * nchunks + e0 / ce : -1, net->ro_pmu + s0 * 2, net->ro_psg + s0 * 2, net->ro_val + s0);
            if (rc) return rc;
        }
    const int apply_update = finish, reduce = finish;      // finish == 0: fold and local statistics only, nothing reduced or applied
    return train_finish(pass, tb, inv_total, apply_update ? lr : 0.f, apply_update, stats_host, reduce);
}

// A gradient step that left the fp16 range (GRL_E_RANGE from train_apply: Adam was skipped on the device, nothing changed) switches
// the net to the fp32-MFMA GEMMs -- every rank does, the flag was max-reduced -- and then
//   * runs the step again when only the backward pass overflowed (the rollout's actions, values and advantages are valid);
//   * gives the update up when the rollout's own forward passes overflowed (its actions came from invalid heads): the call returns
//     GRL_OK with NaN statistics and update_skipped = 1 (grl_net_range_info), the next rollout runs on the fp32 form.
static int train_rollout_checked(grl_net *net, float lr, float *stats_host, int finish) {
    if (net) net->update_skipped_last = 0;
    int rc = train_rollout_impl(net, lr, stats_host, finish);
    if (rc != GRL_E_RANGE) return rc;
    // Under RCCL the flag was max-reduced, so every rank is here together and the decision below must not depend on rank-local state:
    // a rank whose net already computes in fp32 (it fell back alone in a predict() on its own data) joins the retry as a no-op switch
    // instead of returning the error while its peers wait for it in the next all-reduce.
    if (!range_fall_back(net) && !(net->comm && net->range_fallback_on)) return rc;
    if (net->range_bits_last & 2) {
        net->update_skipped_last = 1;
        if (stats_host) for (int i = 0; i < 4; ++i) stats_host[i] = __builtin_nanf("");
        return GRL_OK;
    }
    return train_rollout_impl(net, lr, stats_host, finish);
}

int grl_net_train_rollout(grl_net *net, float lr, float *stats_host) { return train_rollout_checked(net, lr, stats_host, 1); }

int grl_net_train_rollout_grads(grl_net *net, float *stats_host) { return train_rollout_checked(net, 0.f, stats_host, 0); }

int grl_net_set_grads(grl_net *net, const float *host, int64_t cnt) {
    return paac_copy_flat(net, "grl_net_set_grads", net ? net->grads : nullptr, (float *)host, cnt, true);
}

int grl_net_apply_grads(grl_net *net, float lr, float grad_scale, float *stats_host) {
    if (!net || !net->train_ready) return paac_fail(net, GRL_E_STATE, "grl_net_apply_grads: no gradient step has run yet");
    hipSetDevice(net->h->cfg.device_id);
    return train_apply(net, net->last_inv_total, lr, 1, grad_scale, stats_host);
}

static int train_obs_impl(grl_net *net, int32_t n_envs, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, const float *actions,
                          const float *advantages, const float *critic_target, float lr, int32_t apply_update, float *stats_host) {
    if (!net || n_envs <= 0 || !lb || !ab || !pos || !actions || !advantages || !critic_target)
        return paac_fail(net, GRL_E_INVALID, "grl_net_train_obs: bad argument");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = ensure_tmp_obs(net, n_envs);
    if (rc) return rc;
    hipStream_t st0 = net->lane_stream[0];
    PAAC_HIP(net, hipMemcpyAsync(net->tmp_lb, lb, (size_t)n_envs * 160, hipMemcpyHostToDevice, st0));
    PAAC_HIP(net, hipMemcpyAsync(net->tmp_ab, ab, (size_t)n_envs * 20, hipMemcpyHostToDevice, st0));
    PAAC_HIP(net, hipMemcpyAsync(net->tmp_pos, pos, (size_t)n_envs * 20, hipMemcpyHostToDevice, st0));
    TrainBufs tb[GRL_MAX_LANES];
    LanePass pass(net);      // from here on every way out joins: lane 0 and the handle's own stream are current again
    if ((rc = train_begin(net, tb))) return rc;
    const int ce = net->chunk / 10, nl = lanes_active(net);
    const float inv_total = 1.0f / (float)(n_envs * 10);
    // a chunk's actions, advantages and targets into lane buffers t, on stream st
    auto stage = [&](const TrainBufs &t, size_t s0, int ne, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(t.cact, actions + s0 * net->ho.A, (size_t)ne * 10 * net->ho.A * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(t.cadv, advantages + s0, (size_t)ne * 10 * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(t.cy, critic_target + s0, (size_t)ne * 10 * 4, hipMemcpyHostToDevice, st);
        return e == hipSuccess ? GRL_OK : paac_fail(net, GRL_E_HIP, std::string("grl_net_train_obs: hipMemcpyAsync: ") + hipGetErrorString(e));
    };
    // the loss scale needs the heads of every sample before the first backward pass: one forward sweep on lane 0
    for (int e0 = 0; e0 < n_envs; e0 += ce) {
        const int ne = n_envs - e0 < ce ? n_envs - e0 : ce;
        const TrainBufs &t = tb[0];
        if ((rc = stage(t, (size_t)e0 * 10, ne, st0))) return rc;
        bind_activations(net, -1);
        if ((rc = forward_chunk(net, net->tmp_lb + (size_t)e0 * 160, net->tmp_ab + (size_t)e0 * 20, net->tmp_pos + (size_t)e0 * 20, ne, t.cmu,
                                t.csigma, t.cvs)) ||
            (rc = train_bound_rows(net, t.cmu, t.csigma, t.cvs, t.cact, t.cadv, t.cy, (long)ne * 10)))
            return rc;
        PAAC_HIP(net, hipStreamSynchronize(st0));      // host staging buffers are reused by the next chunk
    }
    if ((rc = train_scale_and_fork(net, inv_total))) return rc;
    for (int e0 = 0; e0 < n_envs; e0 += ce) {
        int ne = n_envs - e0 < ce ? n_envs - e0 : ce;
        use_lane(net, (e0 / ce) % nl);
        hipStream_t st = net->h->stream;
        const TrainBufs &t = tb[net->cur_lane];
        if ((rc = stage(t, (size_t)e0 * 10, ne, st)) ||
            (rc = backward_chunk(net, t, net->tmp_lb + (size_t)e0 * 160, net->tmp_ab + (size_t)e0 * 20, net->tmp_pos + (size_t)e0 * 20, ne, t.cact,
                                 t.cadv, t.cy, inv_total)))
            return rc;
        if (hipError_t e = hipStreamSynchronize(st))      // host staging buffers are reused by the next chunk
            return paac_fail(net, GRL_E_HIP, std::string("grl_net_train_obs: hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    return train_finish(pass, tb, inv_total, lr, apply_update, stats_host);
}

int grl_net_train_obs(grl_net *net, int32_t n_envs, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, const float *actions,
                      const float *advantages, const float *critic_target, float lr, int32_t apply_update, float *stats_host) {
    if (net) net->update_skipped_last = 0;
    int rc = train_obs_impl(net, n_envs, lb, ab, pos, actions, advantages, critic_target, lr, apply_update, stats_host);
    if (rc == GRL_E_RANGE && range_fall_back(net))      // forward and backward both run inside the call: all of it once more on the fp32 form
        rc = train_obs_impl(net, n_envs, lb, ab, pos, actions, advantages, critic_target, lr, apply_update, stats_host);
    return rc;
}

int grl_net_host_times(grl_net *net, int64_t *rollouts_out, int64_t *updates_out, double *rollout_enqueue_ms_out,
                       double *train_enqueue_ms_out, double *train_wait_ms_out) {
    if (!net) return GRL_E_INVALID;
    if (rollouts_out) *rollouts_out = net->ht_rollouts;
    if (updates_out) *updates_out = net->ht_updates;
    if (rollout_enqueue_ms_out) *rollout_enqueue_ms_out = net->ht_rollout_ms;
    if (train_enqueue_ms_out) *train_enqueue_ms_out = net->ht_train_enq_ms;
    if (train_wait_ms_out) *train_wait_ms_out = net->ht_train_wait_ms;
    return GRL_OK;
}

int grl_net_keep_info(grl_net *net, int32_t *level_out, int64_t *slots_out, int64_t *slot_bytes_out, int64_t *headroom_bytes_out,
                      int64_t *free_bytes_out, int32_t *resident_out) {
    if (!net) return GRL_E_INVALID;
    if (level_out) *level_out = net->keep ? net->keep_level : 0;
    if (slots_out) *slots_out = net->keep ? (int64_t)net->keep_slots : 0;
    if (slot_bytes_out)
        for (int level = 1; level <= 3; ++level) slot_bytes_out[level - 1] = (int64_t)(keep_floats_per_slot(net, level) * sizeof(float));
    if (headroom_bytes_out) *headroom_bytes_out = (int64_t)net->keep_headroom;
    if (free_bytes_out) *free_bytes_out = (int64_t)net->keep_free_seen;
    if (resident_out) *resident_out = net->resident_last;
    return GRL_OK;
}

int grl_net_get_action_counter(grl_net *net, uint64_t *out) { return paac_get_action_counter(net, out); }
int grl_net_set_action_counter(grl_net *net, uint64_t value) { return paac_set_action_counter(net, value); }

int grl_comm_unique_id(void *out, size_t bytes) {
    if (!out || bytes != sizeof(ncclUniqueId)) return GRL_E_INVALID;
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    (void)hipGetLastError();
    if (r != ncclSuccess) return GRL_E_COMM;
    memcpy(out, &id, sizeof(id));
    return GRL_OK;
}

size_t grl_comm_unique_id_bytes(void) { return sizeof(ncclUniqueId); }

int grl_net_comm_init(grl_net *net, const void *unique_id, size_t bytes, int32_t rank, int32_t world_size) {
    return paac_comm_init(net, "grl_net_comm_init", unique_id, bytes, rank, world_size);
}

int grl_net_comm_info(grl_net *net, int32_t *count_out, int32_t *user_rank_out, int64_t *allreduce_calls_out,
                      double *allreduce_ms_total_out, float *allreduce_ms_last_out) {
    return paac_comm_info(net, count_out, user_rank_out, allreduce_calls_out, allreduce_ms_total_out, allreduce_ms_last_out);
}

int grl_net_comm_broadcast_params(grl_net *net, int32_t root) {
    int rc = paac_comm_broadcast_params(net, "grl_net_comm_broadcast_params", root);
    return rc ? rc : params_moved(net);
}

int grl_net_comm_destroy(grl_net *net) { return paac_comm_destroy(net); }

int grl_net_read_rollout(grl_net *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return GRL_E_INVALID;
    if (!net->ro_lb) return paac_fail(net, GRL_E_STATE, "grl_net_read_rollout: no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    std::string w(which);
    const size_t T = net->T, B = net->B, E = net->h->E;
    const void *src = nullptr;
    size_t need = 0;
    if (w == "actions") { src = net->ro_act; need = T * B * 8; }
    else if (w == "values") { src = net->ro_val; need = T * B * 4; }
    else if (w == "rewards") { src = net->ro_rew; need = T * B * 4; }
    else if (w == "y") { src = net->ro_y; need = T * B * 4; }
    else if (w == "adv") { src = net->ro_adv; need = T * B * 4; }
    else if (w == "boot") { src = net->ro_boot; need = B * 4; }
    else if (w == "locust_bins") { src = net->ro_lb; need = T * E * 160; }
    else if (w == "agent_bins") { src = net->ro_ab; need = T * E * 20; }
    else if (w == "positions") { src = net->ro_pos; need = T * E * 20; }
    else if (w == "dones") { src = net->ro_done; need = T * E; }
    else return paac_fail(net, GRL_E_INVALID, "grl_net_read_rollout: unknown buffer '" + w + "'");
    if (need != bytes) return paac_fail(net, GRL_E_SIZE, "grl_net_read_rollout: '" + w + "' needs " + std::to_string(need) + " bytes");
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    PAAC_HIP(net, hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // extern "C"
