// Evaluation image tail: fused SSIM / squared-error sums and 8-bit frames.
//
// Reference semantics (ShawnnnLiu/Robust-NeRF):
//   compute_ssim / compute_mse     noisy_src/metrics.py:43-116: 11x11 Gaussian window
//       (sigma 1.5), zero padding 5, grouped per channel, blur of p, t, p^2, t^2, p t
//   save_image                     noisy_src/inference.py:108-111: x * 255, clip, uint8
//   depth_to_colormap              noisy_src/inference.py:114-125: min-max normalise, ramp
//
// nr_image_metrics promotes the fp32 pixels to double and does everything after that in
// fp64: E[x^2] - mu^2 sits near 1 against C2 = 9e-4 on the white-background scenes, and
// in fp32 the fifth decimal of the mean SSIM depends on the summation order.  The blur
// is separable (11 taps across, then 11 down), ~130 fp64 FMAs per pixel-channel.
//
// Determinism: no atomics.  Every workgroup reduces in a fixed tree and writes its
// partials to its own workspace slot; a one-workgroup launch sums the slots in a fixed
// order (thread t takes slots t, t + 256, ... in index order, then the same tree).
#include <cfloat>
#include <climits>

#include "common.hpp"

namespace nr {

constexpr int kWin = 11;             // SSIM window
constexpr int kPad = kWin / 2;       // zero padding on every side
constexpr int kTileW = 32;           // output tile of one workgroup
constexpr int kTileH = 16;
constexpr int kHaloW = kTileW + 2 * kPad;  // 42
constexpr int kHaloH = kTileH + 2 * kPad;  // 26
constexpr int kImgThreads = 256;
constexpr int kMaxSlots = INT_MAX / kImgThreads;  // grid * block stays an int
constexpr int kMinMaxBlocks = 256;

struct Gauss11 {
    float w[kWin];
};

// Fixed-shape tree over the workgroup's kImgThreads values (sm: kImgThreads doubles).
__device__ __forceinline__ double block_sum_f64(double v, double* sm) {
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = kImgThreads / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] += sm[t + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// One workgroup per (channel, tile row, tile column); slot = blockIdx.x.
// LDS: 2 x 26 x 42 floats (8,736 B) + 5 x 26 x 32 doubles (33,280 B) + 256 doubles.
__global__ void __launch_bounds__(kImgThreads)
image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H, int W, int C,
                     int tiles_x, int tiles_y, Gauss11 g, double C1, double C2, double* __restrict__ partials) {
    __shared__ float s_p[kHaloH][kHaloW];
    __shared__ float s_t[kHaloH][kHaloW];
    __shared__ double s_h[5][kHaloH][kTileW];
    __shared__ double s_red[kImgThreads];

    const int slot = blockIdx.x;
    const int tx = slot % tiles_x;
    const int ty = (slot / tiles_x) % tiles_y;
    const int c = slot / (tiles_x * tiles_y);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int tid = threadIdx.x;

    // halo of pred / target, zeros outside the image (the reference's zero padding)
    for (int i = tid; i < kHaloH * kHaloW; i += kImgThreads) {
        const int r = i / kHaloW, q = i % kHaloW;
        const int y = y0 + r - kPad, x = x0 + q - kPad;
        float p = 0.f, t = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t o = (static_cast<size_t>(y) * W + x) * C + c;
            p = pred[o];
            t = target[o];
        }
        s_p[r][q] = p;
        s_t[r][q] = t;
    }
    __syncthreads();

    double gw[kWin];
#pragma unroll
    for (int k = 0; k < kWin; ++k) gw[k] = static_cast<double>(g.w[k]);

    // horizontal pass over every halo row
    for (int i = tid; i < kHaloH * kTileW; i += kImgThreads) {
        const int r = i / kTileW, q = i % kTileW;
        double a_p = 0.0, a_t = 0.0, a_pp = 0.0, a_tt = 0.0, a_pt = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const double p = static_cast<double>(s_p[r][q + k]);
            const double t = static_cast<double>(s_t[r][q + k]);
            a_p += gw[k] * p;
            a_t += gw[k] * t;
            a_pp += gw[k] * (p * p);
            a_tt += gw[k] * (t * t);
            a_pt += gw[k] * (p * t);
        }
        s_h[0][r][q] = a_p;
        s_h[1][r][q] = a_t;
        s_h[2][r][q] = a_pp;
        s_h[3][r][q] = a_tt;
        s_h[4][r][q] = a_pt;
    }
    __syncthreads();

    // vertical pass, the SSIM map and the squared error of the tile's own pixels
    double ssim = 0.0, sq = 0.0;
    for (int i = tid; i < kTileH * kTileW; i += kImgThreads) {
        const int r = i / kTileW, q = i % kTileW;
        if (y0 + r < H && x0 + q < W) {
            double mu_p = 0.0, mu_t = 0.0, e_pp = 0.0, e_tt = 0.0, e_pt = 0.0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                mu_p += gw[k] * s_h[0][r + k][q];
                mu_t += gw[k] * s_h[1][r + k][q];
                e_pp += gw[k] * s_h[2][r + k][q];
                e_tt += gw[k] * s_h[3][r + k][q];
                e_pt += gw[k] * s_h[4][r + k][q];
            }
            const double mu_p2 = mu_p * mu_p, mu_t2 = mu_t * mu_t, mu_pt = mu_p * mu_t;
            const double v_p = e_pp - mu_p2, v_t = e_tt - mu_t2, v_pt = e_pt - mu_pt;
            ssim += ((2.0 * mu_pt + C1) * (2.0 * v_pt + C2)) / ((mu_p2 + mu_t2 + C1) * (v_p + v_t + C2));
            const double d = static_cast<double>(s_p[r + kPad][q + kPad]) - static_cast<double>(s_t[r + kPad][q + kPad]);
            sq += d * d;
        }
    }
    const double ssim_sum = block_sum_f64(ssim, s_red);
    const double sq_sum = block_sum_f64(sq, s_red);
    if (tid == 0) {
        partials[2 * static_cast<size_t>(slot)] = ssim_sum;
        partials[2 * static_cast<size_t>(slot) + 1] = sq_sum;
    }
}

__global__ void __launch_bounds__(kImgThreads)
image_metrics_final_kernel(const double* __restrict__ partials, int nslots, double* __restrict__ out) {
    __shared__ double s_red[kImgThreads];
    double ssim = 0.0, sq = 0.0;
    for (int i = threadIdx.x; i < nslots; i += kImgThreads) {
        ssim += partials[2 * static_cast<size_t>(i)];
        sq += partials[2 * static_cast<size_t>(i) + 1];
    }
    const double ssim_sum = block_sum_f64(ssim, s_red);
    const double sq_sum = block_sum_f64(sq, s_red);
    if (threadIdx.x == 0) {
        out[0] = ssim_sum;
        out[1] = sq_sum;
    }
}

// save_image's quantisation: x * 255, clip to [0, 255], truncate; 0 for non-finite x.
__device__ __forceinline__ uint8_t quantise_u8(float x) {
    if (!(fabsf(x) <= FLT_MAX)) return 0;
    float v = x * 255.0f;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return static_cast<uint8_t>(static_cast<int>(v));
}

__global__ void __launch_bounds__(kImgThreads)
frame_u8_kernel(const float* __restrict__ src, int H, int row_elems, uint8_t* __restrict__ dst, int64_t dst_stride,
                int64_t dst_off) {
    const int64_t n = static_cast<int64_t>(H) * row_elems;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kImgThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kImgThreads + threadIdx.x; i < n; i += stride) {
        const int64_t y = i / row_elems, e = i - y * row_elems;
        dst[y * dst_stride + dst_off + e] = quantise_u8(src[i]);
    }
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// Fixed-shape min / max tree over the workgroup (sm: 2 x kImgThreads floats).
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* sm) {
    const int t = threadIdx.x;
    sm[t] = lo;
    sm[kImgThreads + t] = hi;
    __syncthreads();
#pragma unroll
    for (int s = kImgThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            sm[t] = fminf(sm[t], sm[t + s]);
            sm[kImgThreads + t] = fmaxf(sm[kImgThreads + t], sm[kImgThreads + t + s]);
        }
        __syncthreads();
    }
    lo = sm[0];
    hi = sm[kImgThreads];
    __syncthreads();
}

// partials: [0, kMinMaxBlocks) minima, [kMinMaxBlocks, 2 kMinMaxBlocks) maxima; a
// workgroup with no pixel writes +inf / -inf.
__global__ void __launch_bounds__(kImgThreads)
depth_minmax_kernel(const float* __restrict__ depth, int64_t n, float* __restrict__ partials) {
    __shared__ float sm[2 * kImgThreads];
    float lo = INFINITY, hi = -INFINITY;
    const int64_t stride = static_cast<int64_t>(kMinMaxBlocks) * kImgThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kImgThreads + threadIdx.x; i < n; i += stride) {
        const float d = depth[i];
        lo = fminf(lo, d);
        hi = fmaxf(hi, d);
    }
    block_minmax(lo, hi, sm);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = lo;
        partials[kMinMaxBlocks + blockIdx.x] = hi;
    }
}

// Every workgroup reduces the kMinMaxBlocks (== kImgThreads) partials itself, then colours.
__global__ void __launch_bounds__(kImgThreads)
depth_frame_kernel(const float* __restrict__ depth, int64_t n, const float* __restrict__ partials,
                   uint8_t* __restrict__ dst) {
    __shared__ float sm[2 * kImgThreads];
    float lo = partials[threadIdx.x], hi = partials[kMinMaxBlocks + threadIdx.x];
    block_minmax(lo, hi, sm);
    const float den = (hi - lo) + 1e-8f;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kImgThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kImgThreads + threadIdx.x; i < n; i += stride) {
        const float v = __fdiv_rn(depth[i] - lo, den);
        const float r = clamp01(4.0f * v - 1.5f);
        const float g = clamp01(2.0f - 4.0f * fabsf(v - 0.5f));
        const float b = clamp01(1.5f - 4.0f * v);
        dst[3 * i] = quantise_u8(r);
        dst[3 * i + 1] = quantise_u8(g);
        dst[3 * i + 2] = quantise_u8(b);
    }
}

static_assert(kMinMaxBlocks == kImgThreads, "depth_frame_kernel reads one partial pair per thread");

// tiles * C of an H x W x C image, or -1 when the arguments are refused.
static int64_t metrics_slots(int H, int W, int C) {
    if (H < 1 || W < 1 || (C != 1 && C != 3)) return -1;
    return static_cast<int64_t>(ceil_div(W, kTileW)) * ceil_div(H, kTileH) * C;
}

}  // namespace nr

using namespace nr;

extern "C" {

int64_t nr_image_metrics_workspace_bytes(int H, int W, int C) {
    const int64_t slots = metrics_slots(H, W, C);
    if (slots < 0 || slots > kMaxSlots) {
        set_error("nr_image_metrics_workspace_bytes: need H >= 1, W >= 1, C in {1, 3} and at most %d tiles x channels "
                  "(%d x %d tiles), got H=%d W=%d C=%d", kMaxSlots, kTileW, kTileH, H, W, C);
        return -1;
    }
    return slots * 2 * static_cast<int64_t>(sizeof(double));
}

int nr_image_metrics(const float* pred, const float* target, int H, int W, int C, const float* g, double C1, double C2,
                     double* out, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(C == 1 || C == 3, "nr_image_metrics: C must be 1 or 3, got %d", C);
    NR_REQUIRE(H >= 1 && W >= 1, "nr_image_metrics: need H >= 1 and W >= 1, got H=%d W=%d", H, W);
    const int64_t slots = metrics_slots(H, W, C);
    NR_REQUIRE(slots <= kMaxSlots,
               "nr_image_metrics: %lld tiles x channels (%d x %d pixel tiles) exceed the %d slots the partials "
               "workspace indexes with an int", static_cast<long long>(slots), kTileW, kTileH, kMaxSlots);
    NR_REQUIRE(pred && target && g && out && workspace, "nr_image_metrics: null pointer");
    Gauss11 gw;
    for (int k = 0; k < kWin; ++k) gw.w[k] = g[k];
    double* partials = static_cast<double*>(workspace);
    const int tiles_x = ceil_div(W, kTileW), tiles_y = ceil_div(H, kTileH);
    hipLaunchKernelGGL(image_metrics_kernel, dim3(static_cast<unsigned>(slots)), dim3(kImgThreads), 0,
                       static_cast<hipStream_t>(stream), pred, target, H, W, C, tiles_x, tiles_y, gw, C1, C2, partials);
    NR_LAUNCH_CHECK("nr_image_metrics");
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3(1), dim3(kImgThreads), 0, static_cast<hipStream_t>(stream),
                       partials, static_cast<int>(slots), out);
    NR_LAUNCH_CHECK("nr_image_metrics");
    return NR_OK;
}

int nr_frame_u8(const float* src, int H, int W, int C, uint8_t* dst, int64_t dst_stride, int dst_x0,
                nr_stream_t stream) {
    NR_REQUIRE(src && dst, "nr_frame_u8: null pointer");
    NR_REQUIRE(H >= 1 && W >= 1 && C >= 1 && static_cast<int64_t>(W) * C <= INT_MAX,
               "nr_frame_u8: need H >= 1, W >= 1, C >= 1 and W * C <= %d, got H=%d W=%d C=%d", INT_MAX, H, W, C);
    NR_REQUIRE(dst_x0 >= 0 && (static_cast<int64_t>(dst_x0) + W) * C <= dst_stride,
               "nr_frame_u8: columns [%d, %d) x %d channels do not fit a row of dst_stride %lld bytes", dst_x0,
               dst_x0 + W, C, static_cast<long long>(dst_stride));
    const int row = W * C;
    hipLaunchKernelGGL(frame_u8_kernel, dim3(stream_grid(static_cast<long long>(H) * row, kImgThreads)),
                       dim3(kImgThreads), 0, static_cast<hipStream_t>(stream), src, H, row, dst, dst_stride,
                       static_cast<int64_t>(dst_x0) * C);
    NR_LAUNCH_CHECK("nr_frame_u8");
    return NR_OK;
}

int64_t nr_depth_frame_u8_workspace_bytes(void) { return 2 * static_cast<int64_t>(kMinMaxBlocks) * sizeof(float); }

int nr_depth_frame_u8(const float* depth, int H, int W, uint8_t* dst, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(depth && dst && workspace, "nr_depth_frame_u8: null pointer");
    NR_REQUIRE(H >= 1 && W >= 1, "nr_depth_frame_u8: need H >= 1 and W >= 1, got H=%d W=%d", H, W);
    const int64_t n = static_cast<int64_t>(H) * W;
    float* partials = static_cast<float*>(workspace);
    hipLaunchKernelGGL(depth_minmax_kernel, dim3(kMinMaxBlocks), dim3(kImgThreads), 0,
                       static_cast<hipStream_t>(stream), depth, n, partials);
    NR_LAUNCH_CHECK("nr_depth_frame_u8");
    hipLaunchKernelGGL(depth_frame_kernel, dim3(stream_grid(n, kImgThreads)), dim3(kImgThreads), 0,
                       static_cast<hipStream_t>(stream), depth, n, partials, dst);
    NR_LAUNCH_CHECK("nr_depth_frame_u8");
    return NR_OK;
}

}  // extern "C"
