// Included inside namespace grl by net_gated.hip (the Ticker gated trader) and net_gauss.hip (the Gaussian Solow / TradeAR1 agent):
// the device side of the A3C update both share -- float64 sums of squares of [policy P | value P], the clip factors, both RMSProp
// steps.  static: every including translation unit has its own copy.

// sums of squares in float64 of the two gradients: kA3cSumsqBlocks partial sums each, added in order by a3c_finalize_kernel
constexpr int kA3cSumsqBlocks = 32;
static __global__ __launch_bounds__(256) void a3c_sumsq_kernel(const float *__restrict__ g, long n, double *__restrict__ out) {
    __shared__ double red[256];
    const float *gg = g + (size_t)blockIdx.y * n;
    const long per = (n + kA3cSumsqBlocks - 1) / kA3cSumsqBlocks, lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += (double)gg[i] * (double)gg[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.y * kA3cSumsqBlocks + blockIdx.x] = red[0];
}

// stats: policy loss, value loss, entropy mean, policy norm, value norm, lr; then the two clip factors (tf.clip_by_global_norm)
// heads: entropy terms per sample (stats64[2] sums weight * entropy over them)
static __global__ void a3c_finalize_kernel(const double *__restrict__ stats64, const double *__restrict__ sumsq, double heads, float clip_norm,
                                           float lr, float *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sp = 0.0, sv = 0.0;
    for (int b = 0; b < kA3cSumsqBlocks; ++b) { sp += sumsq[b]; sv += sumsq[kA3cSumsqBlocks + b]; }
    const float np_ = (float)sqrt(sp), nv = (float)sqrt(sv);
    stats[0] = (float)stats64[0];
    stats[1] = (float)stats64[1];
    stats[2] = stats64[3] > 0.0 ? (float)(stats64[2] / (heads * stats64[3])) : 0.f;
    stats[3] = np_; stats[4] = nv; stats[5] = lr;
    stats[6] = clip_norm > 0.f ? clip_norm / fmaxf(np_, clip_norm) : 1.0f;
    stats[7] = clip_norm > 0.f ? clip_norm / fmaxf(nv, clip_norm) : 1.0f;
}

// both RMSProp steps (TF 1.x, momentum 0): ms <- rho ms + (1-rho) g^2 ; step = lr g / sqrt(ms + eps).  The policy gradient covers
// [0, v1w), the value gradient [0, c1w) (the trunk) and [v1w, total): the trunk takes both steps, each from the same pre-update parameters.
static __global__ void a3c_rmsprop_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ msp, float *__restrict__ msv, long n,
                                     long c1w, long v1w, const float *__restrict__ stats, float rho, float eps) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float lr = stats[5];
    float w = p[i];
    if (i < v1w) {
        const float gi = g[i] * stats[6];
        const float m = rho * msp[i] + (1.0f - rho) * gi * gi;
        msp[i] = m;
        w = w - lr * gi / sqrtf(m + eps);
    }
    if (i < c1w || i >= v1w) {
        const float gi = g[n + i] * stats[7];
        const float m = rho * msv[i] + (1.0f - rho) * gi * gi;
        msv[i] = m;
        w = w - lr * gi / sqrtf(m + eps);
    }
    p[i] = w;
}

static __global__ void a3c_fill_kernel(float *__restrict__ p, long n, float v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
