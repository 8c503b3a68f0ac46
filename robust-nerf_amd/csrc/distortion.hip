// Distortion regulariser on the ray weights (mip-NeRF 360, Barron et al. 2022, eq. 15).
//
// Per ray, with nondecreasing samples z_0 <= ... <= z_{S-1} in [near, far] and their
// compositing weights w_i (no reference counterpart; additive to ABI 5):
//   s_i = (z_i - near) / (far - near);  e_i = s_i (i < S), e_S = 1
//   m_i = (e_i + e_{i+1}) / 2,  d_i = e_{i+1} - e_i     (the last interval, "infinite" in
//                                                        raw2outputs, is closed at far)
//   L   = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
//   dL/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i
// The m are sorted, so both are exclusive prefix sums.  With W_<i = sum_{j<i} w_j,
// M_<i = sum_{j<i} w_j m_j and the totals W, M:
//   L       = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 d_i
//   dL/dw_i = 2 [m_i (W_<i - W_>i) - (M_<i - M_>i)] + (2/3) w_i d_i
//             W_>i = W - W_<i - w_i,  M_>i = M - M_<i - w_i m_i
// (ties, m_i = m_j, contribute 0 on whichever side they are counted).
//
// One 64-lane wave per ray, four rays per workgroup, lane j owns the contiguous samples
// [jK, jK + K), K = ceil(S / 64): the layout of the wave-per-ray compositing kernels.  Pass
// 1 sums the lane's w and w m; an exclusive wave scan turns them into the lane's prefixes
// and the totals; pass 2 reads the lane's samples again (nothing is held in registers, so
// one form serves every S up to the sampler's 4096), writes the gradient and sums L.
// Everything after the two fp32 loads is fp64: on a converged ray L's terms are ~1e-3
// differences of aggregates of order 1, and the kernel is bound by its 12 B per sample, not
// by the adds.  The batch mean is a second one-workgroup launch over the per-ray fp64
// losses in a fixed order: no atomics, the same bits from run to run.
#include "common.hpp"

namespace nr {

struct DistTerms { double w, m, d; };

// Sample i of the ray at base: z_i arrives in zi (the walk loads every z once per pass).
__device__ __forceinline__ DistTerms dist_terms(const float* weights, const float* z, int64_t base, int i, int S,
                                                float zi, float& z_next, double near, double inv_range) {
    const double e0 = (static_cast<double>(zi) - near) * inv_range;
    double e1 = 1.0;
    if (i + 1 < S) {
        z_next = z[base + i + 1];
        e1 = (static_cast<double>(z_next) - near) * inv_range;
    }
    return {static_cast<double>(weights[base + i]), 0.5 * (e0 + e1), e1 - e0};
}

// Exclusive sum scan of v over the wave's lanes; total = the sum over all 64.
__device__ __forceinline__ double wave_excl_sum_f64(double v, int lane, double& total) {
    double incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    total = __shfl(incl, 63);
    const double e = __shfl_up(incl, 1);
    return lane == 0 ? 0.0 : e;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// g_scale = grad_scale / B: g_w = g_scale * dL/dw.  ray_loss (B doubles) feeds the mean.
__global__ __launch_bounds__(256) void distortion_wave_kernel(const float* __restrict__ weights,
                                                              const float* __restrict__ z, int B, int S, int K,
                                                              double near, double inv_range, double g_scale,
                                                              double* __restrict__ ray_loss,
                                                              float* __restrict__ loss_rays, float* __restrict__ g_w) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;  // wave-uniform; the kernel has no barrier
    const int64_t base = static_cast<int64_t>(b) * S;
    const int i0 = lane * K;
    const int i1 = i0 + K < S ? i0 + K : S;  // lanes past the ray's end walk nothing
    // pass 1: the lane's sums of w and w m
    double sw = 0.0, sm = 0.0;
    float zi = i0 < S ? z[base + i0] : 0.f;
    for (int i = i0; i < i1; ++i) {
        float zn = zi;
        const DistTerms t = dist_terms(weights, z, base, i, S, zi, zn, near, inv_range);
        sw += t.w;
        sm += t.w * t.m;
        zi = zn;
    }
    double W, M;
    double Wl = wave_excl_sum_f64(sw, lane, W);
    double Ml = wave_excl_sum_f64(sm, lane, M);
    // pass 2: the same walk with the running prefixes
    double L = 0.0;
    zi = i0 < S ? z[base + i0] : 0.f;
    for (int i = i0; i < i1; ++i) {
        float zn = zi;
        const DistTerms t = dist_terms(weights, z, base, i, S, zi, zn, near, inv_range);
        const double wm = t.w * t.m;
        const double self = t.w * t.d;
        L += 2.0 * (t.w * (t.m * Wl - Ml)) + self * t.w * (1.0 / 3.0);
        if (g_w) {
            const double Wg = W - Wl - t.w, Mg = M - Ml - wm;
            const double g = 2.0 * (t.m * (Wl - Wg) - (Ml - Mg)) + self * (2.0 / 3.0);
            g_w[base + i] = static_cast<float>(g_scale * g);
        }
        Wl += t.w;
        Ml += wm;
        zi = zn;
    }
    L = wave_sum_f64(L);
    if (lane == 0) {
        ray_loss[b] = L;
        if (loss_rays) loss_rays[b] = static_cast<float>(L);
    }
}

// loss = (sum of the per-ray losses) / B in a fixed order: thread t sums rays t, t + 1024,
// ..., then the xor butterfly within each wave, then the 16 waves in index order.  One block.
__global__ __launch_bounds__(1024) void distortion_mean_kernel(const double* ray_loss, int B, float* loss) {
    __shared__ double part[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < B; i += blockDim.x) s += ray_loss[i];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < 16; ++w) tot += part[w];
        *loss = static_cast<float>(tot / static_cast<double>(B));
    }
}

}  // namespace nr

using namespace nr;

extern "C" {

int64_t nr_distortion_workspace_bytes(int B) { return B > 0 ? int64_t{8} * B : 0; }

int nr_distortion_loss(const float* weights, const float* z, int B, int S, float near, float far, float grad_scale,
                       float* loss, float* loss_rays, float* g_weights, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(B >= 1, "nr_distortion_loss: B = %d rays (at least 1)", B);
    NR_REQUIRE(S >= 1 && S <= 4096, "nr_distortion_loss: S = %d samples per ray (1..4096)", S);
    NR_REQUIRE(far > near, "nr_distortion_loss: far (%g) must exceed near (%g)", static_cast<double>(far),
               static_cast<double>(near));
    NR_REQUIRE(weights && z && loss && workspace, "nr_distortion_loss: weights, z, loss and workspace must not be null");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    double* ray_loss = static_cast<double*>(workspace);
    const double dn = static_cast<double>(near);
    const double inv_range = 1.0 / (static_cast<double>(far) - dn);
    hipLaunchKernelGGL(distortion_wave_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, s, weights, z, B, S, ceil_div(S, 64),
                       dn, inv_range, static_cast<double>(grad_scale) / static_cast<double>(B), ray_loss, loss_rays,
                       g_weights);
    NR_LAUNCH_CHECK("nr_distortion_loss");
    hipLaunchKernelGGL(distortion_mean_kernel, dim3(1), dim3(1024), 0, s, ray_loss, B, loss);
    NR_LAUNCH_CHECK("nr_distortion_loss (mean)");
    return NR_OK;
}

}  // extern "C"
