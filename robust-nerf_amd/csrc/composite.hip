// Volume-rendering alpha composite (forward + backward) and the MSE loss seed.
//
// Reference semantics (ShawnnnLiu/Robust-NeRF):
//   raw2outputs  noisy_src/rendering.py:20-116
//   loss         noisy_src/train.py:89,98 (mean((rgb - target)^2))
//   delta_i = (z_{i+1} - z_i | 1e10) * |d|;  a_i = 1 - exp(-relu(sigma_i + n_i) * delta_i)
//   T_0 = 1, T_{i+1} = T_i * (1 - a_i + 1e-10);  w_i = a_i T_i
//   rgb = sum w c (+ 1 - acc if white), depth = sum w z, acc = sum w.
// Backward uses the division-free form of torch's cumprod gradient:
//   dL/da_i = T_i (G_i - R_i),  R_i = G_{i+1} a_{i+1} + t_{i+1} R_{i+1},  R_{S-1} = 0
// (equal to G_i T_i - (sum_{k>i} G_k w_k) / t_i, the formula autograd evaluates).
//
// Every expression is written once, as a __device__ piece, and the kernels only order them:
//   thread per ray  composite_fwd_kernel, composite_bwd_kernel (S > 64 kCompK): the serial
//                   walk, the transmittance the same sequential product as torch's CPU cumprod
//   wave per ray    gather_lane -> wave_excl_product -> forward_sums    composite_fwd_wave_kernel
//                   gather_lane -> wave_excl_product -> backward_tail   composite_bwd_wave_kernel
//                   all four, with the loss seed before the tail        composite_mse_wave_kernel
// Seams: gather_lane's per-sample hook (the backward computes G there, the fused kernel keeps
// colour and z in registers); forward_sums' colour / z source (memory or those registers);
// backward_tail's Seed and G, passed as values, so absent upstream gradients are the zeros the
// separate kernels read.  The photometric loss is the "loss seed" lines of composite_mse_ray,
// a compile-time member of the robust family (robust_weight, robust_rho):
// composite_mse_wave_kernel is its MSE, composite_robust_wave_kernel<KIND> the others, with a
// second loss word.  A wave form for longer rays is a loop around the same pieces that carries
// E and X from one segment of 64 kCompK samples to the next.
// Host side: those two kernels stay twins (one argument list would change the MSE kernel's
// code); their entry points are argument checks around one body, composite_train.
#include <cmath>

#include "common.hpp"

namespace nr {

struct SampleTerms {
    float delta_raw, alpha, e, sig, t;  // sig = relu'd sigma after noise, t = 1 - alpha + 1e-10
};

__device__ __forceinline__ SampleTerms sample_terms(const float* sigma, const float* z, const float* noise,
                                                    int64_t base, int i, int S, float dnorm) {
    SampleTerms t;
    t.delta_raw = i < S - 1 ? z[base + i + 1] - z[base + i] : 1e10f;
    float s = sigma[base + i];
    if (noise) s = s + noise[base + i];
    t.sig = s > 0.f ? s : 0.f;
    t.e = expf(-t.sig * (t.delta_raw * dnorm));
    t.alpha = 1.0f - t.e;
    t.t = 1.0f - t.alpha + 1e-10f;
    return t;
}

// ---- per-ray pieces, shared by the thread-per-ray and the wave-per-ray kernels
struct Ray {
    int b;
    int64_t base;  // b * S: the global index of the ray's first sample
    float dx, dy, dz, dnorm;
};

__device__ __forceinline__ Ray load_ray(const float* rd, int b, int S) {
    Ray r;
    r.b = b;
    r.base = static_cast<int64_t>(b) * S;
    r.dx = rd[3 * b], r.dy = rd[3 * b + 1], r.dz = rd[3 * b + 2];
    r.dnorm = norm3(r.dx, r.dy, r.dz);
    return r;
}

// The upstream gradients of one ray; the white background folds -(gr + gg + gb) into ga.
struct Seed { float gr, gg, gb, gd, ga; };

__device__ __forceinline__ Seed upstream_seed(float gr, float gg, float gb, float gd, float g_acc, int white) {
    return {gr, gg, gb, gd, g_acc - (white ? (gr + gg) + gb : 0.f)};
}

__device__ __forceinline__ Seed load_seed(const float* g_map, const float* g_depth, const float* g_acc, int b,
                                          int white) {
    return upstream_seed(g_map[3 * b], g_map[3 * b + 1], g_map[3 * b + 2], g_depth ? g_depth[b] : 0.f,
                         g_acc ? g_acc[b] : 0.f, white);
}

struct ColourZ { float c0, c1, c2, z; };

__device__ __forceinline__ ColourZ load_colour_z(const float* rgb, const float* z, int64_t i) {
    return {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], z[i]};
}

// G_i = dL/dw_i of sample i (global index i for the optional g_w).
__device__ __forceinline__ float upstream_G(const Seed& sd, const ColourZ& s, const float* g_w, int64_t i) {
    float G = ((sd.gr * s.c0 + sd.gg * s.c1) + sd.gb * s.c2) + sd.gd * s.z + sd.ga;
    if (g_w) G += g_w[i];
    return G;
}

struct Maps { float r, g, bl, d, a; };

__device__ __forceinline__ void accumulate(Maps& m, float w, const ColourZ& s) {
    m.r += w * s.c0, m.g += w * s.c1, m.bl += w * s.c2;
    m.d += w * s.z, m.a += w;
}

__device__ __forceinline__ void white_fixup(Maps& m, int white) {
    if (white) m.r = m.r + (1.0f - m.a), m.g = m.g + (1.0f - m.a), m.bl = m.bl + (1.0f - m.a);
}

__device__ __forceinline__ void store_maps(const Maps& m, int b, float* rgb_map, float* depth, float* acc) {
    rgb_map[3 * b] = m.r, rgb_map[3 * b + 1] = m.g, rgb_map[3 * b + 2] = m.bl;
    if (depth) depth[b] = m.d;
    if (acc) acc[b] = m.a;
}

// The gradient stores of sample i (global index) from its transmittance Ti and its
// recurrence value R; the sample's term of g_norm goes to gn64 (see wave_sum_f64).
__device__ __forceinline__ void store_sample_grads(const Seed& sd, float dnorm, int64_t i, float Ti,
                                                   const SampleTerms& st, float G, float R, float* g_rgb,
                                                   float* g_sigma, bool want_norm, double& gn64) {
    const float w = st.alpha * Ti;
    g_rgb[3 * i] = sd.gr * w, g_rgb[3 * i + 1] = sd.gg * w, g_rgb[3 * i + 2] = sd.gb * w;
    const float g_alpha = Ti * (G - R);
    // alpha = 1 - exp(x), x = -relu(s) * delta_raw * |d|
    const float g_x = -g_alpha * st.e;
    g_sigma[i] = (st.sig > 0.f) ? -g_x * (st.delta_raw * dnorm) : 0.f;
    if (want_norm) gn64 += static_cast<double>(g_x * (-st.sig * st.delta_raw));
}

__device__ __forceinline__ void add_g_rd(float* g_rd, const Ray& ray, float g_norm) {
    g_rd[3 * ray.b] += g_norm * ray.dx / ray.dnorm;
    g_rd[3 * ray.b + 1] += g_norm * ray.dy / ray.dnorm;
    g_rd[3 * ray.b + 2] += g_norm * ray.dz / ray.dnorm;
}

__global__ void composite_fwd_kernel(const float* rgb, const float* sigma, const float* z, const float* rd,
                                     const float* noise, int B, int S, int white, float* rgb_map, float* depth,
                                     float* acc, float* weights) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Ray ray = load_ray(rd, b, S);
    float T = 1.0f;
    Maps m = {};
    for (int i = 0; i < S; ++i) {
        const SampleTerms st = sample_terms(sigma, z, noise, ray.base, i, S, ray.dnorm);
        const float w = st.alpha * T;
        T = T * st.t;
        if (weights) weights[ray.base + i] = w;
        accumulate(m, w, load_colour_z(rgb, z, ray.base + i));
    }
    white_fixup(m, white);
    store_maps(m, b, rgb_map, depth, acc);
}

// g_sigma doubles as scratch for T_i between the two passes.
__global__ void composite_bwd_kernel(const float* rgb, const float* sigma, const float* z, const float* rd,
                                     const float* noise, int B, int S, int white, const float* g_map,
                                     const float* g_depth, const float* g_acc, const float* g_w, float* g_rgb,
                                     float* g_sigma, float* g_rd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Ray ray = load_ray(rd, b, S);
    const Seed sd = load_seed(g_map, g_depth, g_acc, b, white);
    // pass 1: transmittance T_i -> g_sigma scratch
    float T = 1.0f;
    for (int i = 0; i < S; ++i) {
        const SampleTerms st = sample_terms(sigma, z, noise, ray.base, i, S, ray.dnorm);
        g_sigma[ray.base + i] = T;
        T = T * st.t;
    }
    // pass 2: reverse recurrence
    float R = 0.f, Gn = 0.f, an = 0.f, tn = 0.f;
    double gn64 = 0.0;  // g_norm, summed in fp64 as in the wave kernels (wave_sum_f64)
    for (int i = S - 1; i >= 0; --i) {
        const SampleTerms st = sample_terms(sigma, z, noise, ray.base, i, S, ray.dnorm);
        const float Ti = g_sigma[ray.base + i];
        const float G = upstream_G(sd, load_colour_z(rgb, z, ray.base + i), g_w, ray.base + i);
        if (i < S - 1) R = Gn * an + tn * R;
        store_sample_grads(sd, ray.dnorm, ray.base + i, Ti, st, G, R, g_rgb, g_sigma, g_rd != nullptr, gn64);
        Gn = G;
        an = st.alpha;
        tn = st.t;
    }
    if (g_rd) add_g_rd(g_rd, ray, static_cast<float>(gn64));
}

// ---- wave-per-ray pieces (S <= 64 * kCompK): one 64-lane wave per ray, lane j
// owns samples [jK, jK + K) (K = ceil(S / 64)), all loads contiguous per lane.
// Transmittance: lane-local running product times the wave's exclusive product
// scan of the per-lane products (the thread-per-ray kernels above walk the ray
// serially through strided loads: 64 rays per launch-wide wave set, latency-bound).
// The backward's reverse recurrence R_i = u_{i+1} + t_{i+1} R_{i+1} (u = G a)
// becomes a lane-local affine map R_i = A_i + B_i X_j of the lane's boundary value
// X_j, and X_j = alpha_{j+1} + beta_{j+1} X_{j+1} is a suffix scan of affine maps
// across lanes.  Samples past S are padded with a = 0, t = 1, G = 0.  Only the
// association of the products and sums differs from the serial walk.
constexpr int kCompK = 8;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// dL/d|d| = sum_i g_x_i (-sigma_i delta_i) is a sum of S signed fp32 products that
// largely cancel, and one number per ray carries the whole g_rays_d: summed in fp32 its
// error was set by the accumulation, not by the terms (6.9 half-ulps of the result at
// S = 512 against 0.4 for the same terms summed in fp64, tests/test_edge_shapes.py).  The
// products stay fp32; only their sum runs in fp64, one add per sample and six shuffles
// per ray, in every backward kernel alike, and only when g_rays_d is wanted.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The lane's K samples and the lane-local product L of the t before each of them.
struct Lane {
    SampleTerms s[kCompK];
    float L[kCompK];
};

// Fills ln for samples [i0, i0 + K) and returns the lane's product of t; hook(k, i) runs
// once per live sample with its global index i.
template <class Hook>
__device__ __forceinline__ float gather_lane(Lane& ln, const float* sigma, const float* z, const float* noise,
                                             const Ray& ray, int i0, int S, int K, Hook&& hook) {
    float P = 1.0f;
#pragma unroll
    for (int k = 0; k < kCompK; ++k) {
        ln.s[k] = {0.f, 0.f, 1.0f, 0.f, 1.0f};  // past S: delta_raw = 0, a = 0, e = 1, sig = 0, t = 1
        ln.L[k] = P;
        const int i = i0 + k;
        if (k < K && i < S) {
            ln.s[k] = sample_terms(sigma, z, noise, ray.base, i, S, ray.dnorm);
            hook(k, ray.base + i);
            P = P * ln.s[k].t;
        }
    }
    return P;
}

// Exclusive product scan of P over the wave's lanes.
__device__ __forceinline__ float wave_excl_product(float P, int lane) {
    float incl = P;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(incl, d);
        if (lane >= d) incl *= o;
    }
    const float E = __shfl_up(incl, 1);
    return lane == 0 ? 1.0f : E;
}

// The ray's maps, the same in every lane; src(k, i) gives the colour and z of sample k.
template <class Src>
__device__ __forceinline__ Maps forward_sums(const Lane& ln, float E, const Ray& ray, int i0, int S, int K,
                                             int white, float* weights, Src&& src) {
    Maps m = {};
#pragma unroll
    for (int k = 0; k < kCompK; ++k) {
        const int i = i0 + k;
        if (k < K && i < S) {
            const float w = ln.s[k].alpha * (E * ln.L[k]);
            if (weights) weights[ray.base + i] = w;
            accumulate(m, w, src(k, ray.base + i));
        }
    }
    m.r = wave_sum(m.r), m.g = wave_sum(m.g), m.bl = wave_sum(m.bl);
    m.d = wave_sum(m.d), m.a = wave_sum(m.a);
    white_fixup(m, white);
    return m;
}

// g_rgb, g_sigma and the ray's g_rd from the lane's G (0 past S) and the seed.
__device__ __forceinline__ void backward_tail(const Lane& ln, const float (&GG)[kCompK], float E, const Ray& ray,
                                              const Seed& sd, int i0, int S, int K, int lane, float* g_rgb,
                                              float* g_sigma, float* g_rd) {
    // lane-local affine maps R_i = A_i + B_i X (X = R at the lane's last sample)
    float A[kCompK], Bc[kCompK];
    float an = 0.f, bn = 1.0f;
#pragma unroll
    for (int k = kCompK - 1; k >= 0; --k) {
        if (k < K) {
            if (k == K - 1) {
                an = 0.f;
                bn = 1.0f;
            } else {
                an = GG[k + 1] * ln.s[k + 1].alpha + ln.s[k + 1].t * an;
                bn = ln.s[k + 1].t * bn;
            }
        }
        A[k] = an;
        Bc[k] = bn;
    }
    // this lane's map for its predecessor: X_{j-1} = alpha + beta X_j
    float qa = GG[0] * ln.s[0].alpha + ln.s[0].t * A[0];
    float qb = ln.s[0].t * Bc[0];
    // suffix composition Q_j = N_j o N_{j+1} o ... o N_63
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float oa = __shfl_down(qa, d), ob = __shfl_down(qb, d);
        if (lane + d < 64) {
            qa = qa + qb * oa;
            qb = qb * ob;
        }
    }
    float X = __shfl_down(qa, 1);
    if (lane == 63) X = 0.f;
    double gn64 = 0.0;  // g_norm: see wave_sum_f64
#pragma unroll
    for (int k = 0; k < kCompK; ++k) {
        const int i = i0 + k;
        if (k < K && i < S)  // g_rd is launch-uniform
            store_sample_grads(sd, ray.dnorm, ray.base + i, E * ln.L[k], ln.s[k], GG[k], A[k] + Bc[k] * X, g_rgb,
                               g_sigma, g_rd != nullptr, gn64);
    }
    const float g_norm = g_rd ? static_cast<float>(wave_sum_f64(gn64)) : 0.f;
    if (g_rd && lane == 0) add_g_rd(g_rd, ray, g_norm);
}

__global__ __launch_bounds__(256) void composite_fwd_wave_kernel(const float* rgb, const float* sigma,
                                                                 const float* z, const float* rd,
                                                                 const float* noise, int B, int S, int K,
                                                                 int white, float* rgb_map, float* depth,
                                                                 float* acc, float* weights) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;  // wave-uniform
    const Ray ray = load_ray(rd, b, S);
    Lane ln;
    const float P = gather_lane(ln, sigma, z, noise, ray, lane * K, S, K, [](int, int64_t) {});
    const float E = wave_excl_product(P, lane);
    const Maps m = forward_sums(ln, E, ray, lane * K, S, K, white, weights,
                                [&](int, int64_t i) { return load_colour_z(rgb, z, i); });
    if (lane == 0) store_maps(m, b, rgb_map, depth, acc);
}

__global__ __launch_bounds__(256) void composite_bwd_wave_kernel(
    const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise, int B, int S, int K,
    int white, const float* g_map, const float* g_depth, const float* g_acc, const float* g_w, float* g_rgb,
    float* g_sigma, float* g_rd) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;  // wave-uniform
    const Ray ray = load_ray(rd, b, S);
    const Seed sd = load_seed(g_map, g_depth, g_acc, b, white);
    Lane ln;
    float GG[kCompK] = {};
    const float P = gather_lane(ln, sigma, z, noise, ray, lane * K, S, K, [&](int k, int64_t i) {
        GG[k] = upstream_G(sd, load_colour_z(rgb, z, i), g_w, i);
    });
    const float E = wave_excl_product(P, lane);
    backward_tail(ln, GG, E, ray, sd, lane * K, S, K, lane, g_rgb, g_sigma, g_rd);
}

__device__ __forceinline__ float mse_grad(float d, float inv, float scale) { return (2.0f * d) * inv * scale; }

// ---- the photometric loss family (include/nerf_hip.h, NR_LOSS_*): per colour channel,
// d = rgb_map - target, scale c > 0, every rho normalised to d^2 for |d| << c, and
// rho' = 2 d w with the IRLS weight w.  fp32 operation order (tests/robust_ref.py restates
// it; the build has no contraction, / and sqrtf are correctly rounded):
//   d2 = d * d;  u = d / c;  q = u * u
//   mse            rho = d2                                w = 1
//   huber          a = |d|;  a <= c: rho = d2              w = 1.0f (literal: the MSE's bits)
//                            else    rho = (2c) a - c c    w = c / a
//   charbonnier    s = sqrtf(1 + q);  rho = (2 d2) / (1 + s)     w = 1 / s
//   cauchy         rho = (c c) log1pf(q)                   w = 1 / (1 + q)
//   geman_mcclure  t = 1 + q;  rho = d2 / t                w = 1 / (t t)
// The seed is mse_grad(d, inv, scale) * w (no multiply at all for mse).
// robust_weight runs in every lane (the seed), robust_rho where the loss is stored.
template <int KIND>
__device__ __forceinline__ float robust_q(float d, float c) {
    const float u = d / c;
    return u * u;
}

template <int KIND>
__device__ __forceinline__ float robust_weight(float d, float c) {
    static_assert(KIND >= NR_LOSS_MSE && KIND <= NR_LOSS_GEMAN_MCCLURE, "unknown loss kind");
    if constexpr (KIND == NR_LOSS_MSE) {
        return 1.0f;
    } else if constexpr (KIND == NR_LOSS_HUBER) {
        const float a = fabsf(d);
        return a <= c ? 1.0f : c / a;
    } else if constexpr (KIND == NR_LOSS_CHARBONNIER) {
        return 1.0f / sqrtf(1.0f + robust_q<KIND>(d, c));
    } else if constexpr (KIND == NR_LOSS_CAUCHY) {
        return 1.0f / (1.0f + robust_q<KIND>(d, c));
    } else {
        const float t = 1.0f + robust_q<KIND>(d, c);
        return 1.0f / (t * t);
    }
}

template <int KIND>
__device__ __forceinline__ float robust_rho(float d, float c) {
    const float d2 = d * d;
    if constexpr (KIND == NR_LOSS_MSE) {
        return d2;
    } else if constexpr (KIND == NR_LOSS_HUBER) {
        const float a = fabsf(d);
        return a <= c ? d2 : (2.0f * c) * a - c * c;
    } else if constexpr (KIND == NR_LOSS_CHARBONNIER) {
        return (2.0f * d2) / (1.0f + sqrtf(1.0f + robust_q<KIND>(d, c)));
    } else if constexpr (KIND == NR_LOSS_CAUCHY) {
        return (c * c) * log1pf(robust_q<KIND>(d, c));
    } else {
        return d2 / (1.0f + robust_q<KIND>(d, c));
    }
}

// mse_grad times the weight; no multiply at all for the MSE.
template <int KIND>
__device__ __forceinline__ float robust_grad(float d, float c, float inv, float scale) {
    if constexpr (KIND == NR_LOSS_MSE) return mse_grad(d, inv, scale);
    else return mse_grad(d, inv, scale) * robust_weight<KIND>(d, c);
}

// One ray of the fused wave kernels (lane = the wave's lane).  No early return here:
// the wave still has to reach the barriers of sum_loss_last_block.  rho_ray (the ray's
// sum of rho) is written only when it is not NULL; composite_mse_wave_kernel passes a
// literal NULL, so its code is the MSE's alone.
template <int KIND>
__device__ __forceinline__ void composite_mse_ray(const float* rgb, const float* sigma, const float* z, const float* rd,
                                                  const float* noise, const float* target, int b, int S, int K,
                                                  int white, float inv, float scale, float c, float* rgb_map,
                                                  float* depth, float* acc, float* weights, float* sqerr,
                                                  float* rho_ray, float* g_rgb, float* g_sigma, float* g_rd,
                                                  int lane) {
    const Ray ray = load_ray(rd, b, S);
    const int i0 = lane * K;
    Lane ln;
    ColourZ cz[kCompK] = {};
    const float P = gather_lane(ln, sigma, z, noise, ray, i0, S, K,
                                [&](int k, int64_t i) { cz[k] = load_colour_z(rgb, z, i); });
    const float E = wave_excl_product(P, lane);
    const Maps m = forward_sums(ln, E, ray, i0, S, K, white, weights, [&](int k, int64_t) { return cz[k]; });
    // loss seed
    const float d0 = m.r - target[3 * b], d1 = m.g - target[3 * b + 1], d2 = m.bl - target[3 * b + 2];
    const Seed sd = upstream_seed(robust_grad<KIND>(d0, c, inv, scale), robust_grad<KIND>(d1, c, inv, scale),
                                  robust_grad<KIND>(d2, c, inv, scale), 0.f, 0.f, white);
    if (lane == 0) {
        store_maps(m, b, rgb_map, depth, acc);
        sqerr[b] = (d0 * d0 + d1 * d1) + d2 * d2;
        if (rho_ray) rho_ray[b] = (robust_rho<KIND>(d0, c) + robust_rho<KIND>(d1, c)) + robust_rho<KIND>(d2, c);
    }
    // backward (composite_bwd_wave_kernel with g_depth = g_acc = g_w = 0)
    float GG[kCompK];
#pragma unroll
    for (int k = 0; k < kCompK; ++k) {
        GG[k] = 0.f;
        if (k < K && i0 + k < S) GG[k] = upstream_G(sd, cz[k], nullptr, 0);
    }
    backward_tail(ln, GG, E, ray, sd, i0, S, K, lane, g_rgb, g_sigma, g_rd);
}

// Sum of v over the workgroup in a fixed order: xor butterfly within each wave, lane 0 of
// each wave to part[wave], one barrier, the waves added in index order from 0.f.  The
// result is thread 0's alone; part holds at least blockDim.x / 64 floats.
__device__ __forceinline__ float block_sum_ordered(float v, float* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float tot = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) tot += part[w];
    return tot;
}

// The last workgroup to finish (an agent-scope ticket; the recipe of
// cdna_hip_programming.md §6 Guideline 16: plain stores, release fence, relaxed
// fetch_add, acquire fence in the reducer) sums the per-ray squared errors in a fixed
// order and leaves the ticket at 0 for the next call.  TWO: the robust form, which sums
// rho_ray as well under the same ticket draw and writes loss[0..1] = {mean rho, mean d^2}.
template <bool TWO>
__device__ __forceinline__ void sum_loss_last_block(const float* sqerr, const float* rho_ray, int B, float inv,
                                                    unsigned* ticket, float* loss) {
    __shared__ float part[5];  // [0..3]: wave sums, [4]: the "last" flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        part[4] = t == gridDim.x - 1 ? 1.f : 0.f;
    }
    __syncthreads();
    if (part[4] == 0.f) return;  // workgroup-uniform
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    float sum = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) sum += sqerr[i];
    if constexpr (TWO) {
        __shared__ float part_rho[4];
        float sum_rho = 0.f;
        for (int i = threadIdx.x; i < B; i += blockDim.x) sum_rho += rho_ray[i];
        const float tot_rho = block_sum_ordered(sum_rho, part_rho);
        if (threadIdx.x == 0) loss[0] = tot_rho * inv;
        ++loss;
    }
    const float tot = block_sum_ordered(sum, part);
    if (threadIdx.x == 0) {
        *loss = tot * inv;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Training form: raw2outputs (rendering.py:20-116) + the MSE loss seed (train.py:89,98:
// mean over 3B of (rgb_map - target)^2, gradient 2 (rgb_map - target) / 3B * scale) + the
// backward of both, in one wave-per-ray pass.  It runs the pieces the forward and the
// backward wave kernels run, with mse_kernel's mse_grad in between (the backward's depth /
// acc / weight terms are the zeros those kernels read for absent gradients), so g_rgb /
// g_sigma / g_rd are bit-identical to the three launches.  The loss is summed per ray
// (sqerr), then over the rays by the last workgroup (ticket) or, without a ticket, by
// loss_sum_kernel.  Dead waves of the last workgroup skip the ray but not the loss sum.
// Two waves per SIMD, as the kernel ran when its 254 registers allowed no more: a step's
// 1,024 workgroups are 16 waves per CU, two even rounds; at the three that its 138 registers
// would allow, the second round runs one wave (measured at S = 192: 17.9 against 17.0 us).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void composite_mse_wave_kernel(
    const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise, const float* target,
    int B, int S, int K, int white, float inv, float scale, float* rgb_map, float* depth, float* acc, float* weights,
    float* sqerr, float* g_rgb, float* g_sigma, float* g_rd, unsigned* ticket, float* loss) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b < B)
        composite_mse_ray<NR_LOSS_MSE>(rgb, sigma, z, rd, noise, target, b, S, K, white, inv, scale, 0.f, rgb_map,
                                       depth, acc, weights, sqerr, nullptr, g_rgb, g_sigma, g_rd, lane);
    if (ticket) sum_loss_last_block<false>(sqerr, nullptr, B, inv, ticket, loss);
}

// The same launch with another member of the loss family in the seed (robust_grad) and
// two loss words: loss2 = {mean rho, mean d^2}, from the per-ray sums rho_ray and sqerr.
// NR_LOSS_MSE here writes d^2 to both arrays, so its two words are the same bits.
template <int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void composite_robust_wave_kernel(
    const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise, const float* target,
    int B, int S, int K, int white, float inv, float scale, float c, float* rgb_map, float* depth, float* acc,
    float* weights, float* sqerr, float* rho_ray, float* g_rgb, float* g_sigma, float* g_rd, unsigned* ticket,
    float* loss2) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b < B) composite_mse_ray<KIND>(rgb, sigma, z, rd, noise, target, b, S, K, white, inv, scale, c, rgb_map, depth,
                                       acc, weights, sqerr, rho_ray, g_rgb, g_sigma, g_rd, lane);
    if (ticket) sum_loss_last_block<true>(sqerr, rho_ray, B, inv, ticket, loss2);
}

// loss = inv * sum of the per-ray squared errors, in a fixed order.  One block.
__global__ __launch_bounds__(1024) void loss_sum_kernel(const float* sqerr, int B, float inv, float* loss) {
    __shared__ float part[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) s += sqerr[i];
    const float tot = block_sum_ordered(s, part);
    if (threadIdx.x == 0) *loss = tot * inv;
}

// loss2 = inv * {sum rho_ray, sum sqerr}, each in loss_sum_kernel's order.  One block.
__global__ __launch_bounds__(1024) void loss2_sum_kernel(const float* rho_ray, const float* sqerr, int B, float inv,
                                                         float* loss2) {
    __shared__ float part_rho[16], part[16];
    float sr = 0.f, s = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) sr += rho_ray[i], s += sqerr[i];
    const float tot_rho = block_sum_ordered(sr, part_rho);
    const float tot = block_sum_ordered(s, part);
    if (threadIdx.x == 0) loss2[0] = tot_rho * inv, loss2[1] = tot * inv;
}

// loss = mean((p - t)^2) over n = 3B; g = 2 (p - t) / n * scale.  One block.
__global__ void mse_kernel(const float* p, const float* t, int n, float scale, float* loss, float* g) {
    __shared__ float part[16];
    float s = 0.f;
    const float inv = 1.0f / static_cast<float>(n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = p[i] - t[i];
        s += d * d;
        if (g) g[i] = mse_grad(d, inv, scale);
    }
    const float tot = block_sum_ordered(s, part);
    if (threadIdx.x == 0 && loss) *loss = tot * inv;
}

// mse_kernel for the loss family: loss2 = {mean rho, mean d^2} over n = 3B (each summed in
// mse_kernel's order), g = mse_grad * w.  One block.
template <int KIND>
__global__ void robust_kernel(const float* p, const float* t, int n, float c, float scale, float* loss2, float* g) {
    __shared__ float part_rho[16], part[16];
    float sr = 0.f, s = 0.f;
    const float inv = 1.0f / static_cast<float>(n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = p[i] - t[i];
        sr += robust_rho<KIND>(d, c);
        s += d * d;
        if (g) g[i] = robust_grad<KIND>(d, c, inv, scale);
    }
    const float tot_rho = block_sum_ordered(sr, part_rho);
    const float tot = block_sum_ordered(s, part);
    if (threadIdx.x == 0 && loss2) loss2[0] = tot_rho * inv, loss2[1] = tot * inv;
}

// Wave per ray up to 64 * kCompK samples (K per lane, four rays per workgroup), thread
// per ray beyond.
struct CompositeForm {
    bool wave;
    int K;
    dim3 grid, block;
};

static CompositeForm composite_form(int B, int S) {
    const bool wave = S <= 64 * kCompK;
    return {wave, (S + 63) / 64, dim3(ceil_div(B, wave ? 4 : 64)), dim3(wave ? 256 : 64)};
}

}  // namespace nr

using namespace nr;

extern "C" {

int nr_composite_fwd(const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise, int B,
                     int S, int white, float* rgb_map, float* depth, float* acc, float* weights,
                     nr_stream_t stream) {
    NR_REQUIRE(rgb && sigma && z && rd && rgb_map && B >= 0 && S > 0, "nr_composite_fwd: bad arguments");
    if (B == 0) return NR_OK;
    const CompositeForm f = composite_form(B, S);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (f.wave)
        hipLaunchKernelGGL(composite_fwd_wave_kernel, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, B, S, f.K, white,
                           rgb_map, depth, acc, weights);
    else
        hipLaunchKernelGGL(composite_fwd_kernel, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, B, S, white, rgb_map,
                           depth, acc, weights);
    NR_LAUNCH_CHECK("nr_composite_fwd");
    return NR_OK;
}

int nr_composite_bwd(const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise, int B,
                     int S, int white, const float* g_map, const float* g_depth, const float* g_acc,
                     const float* g_w, float* g_rgb, float* g_sigma, float* g_rd, nr_stream_t stream) {
    NR_REQUIRE(rgb && sigma && z && rd && g_map && g_rgb && g_sigma && B >= 0 && S > 0,
               "nr_composite_bwd: bad arguments");
    if (B == 0) return NR_OK;
    const CompositeForm f = composite_form(B, S);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (f.wave)
        hipLaunchKernelGGL(composite_bwd_wave_kernel, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, B, S, f.K, white,
                           g_map, g_depth, g_acc, g_w, g_rgb, g_sigma, g_rd);
    else
        hipLaunchKernelGGL(composite_bwd_kernel, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, B, S, white, g_map,
                           g_depth, g_acc, g_w, g_rgb, g_sigma, g_rd);
    NR_LAUNCH_CHECK("nr_composite_bwd");
    return NR_OK;
}

int nr_mse_fwd_bwd(const float* pred, const float* target, int B, float scale, float* loss, float* g,
                   nr_stream_t stream) {
    NR_REQUIRE(pred && target && B > 0, "nr_mse_fwd_bwd: bad arguments");
    hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), pred, target, 3 * B,
                       scale, loss, g);
    NR_LAUNCH_CHECK("nr_mse_fwd_bwd");
    return NR_OK;
}

// kind, launch-uniform, picks the instantiation on the host.
#define NR_LOSS_DISPATCH(kind, LAUNCH)                               \
    switch (kind) {                                                  \
        case NR_LOSS_MSE: LAUNCH(NR_LOSS_MSE); break;                \
        case NR_LOSS_HUBER: LAUNCH(NR_LOSS_HUBER); break;            \
        case NR_LOSS_CHARBONNIER: LAUNCH(NR_LOSS_CHARBONNIER); break; \
        case NR_LOSS_CAUCHY: LAUNCH(NR_LOSS_CAUCHY); break;          \
        default: LAUNCH(NR_LOSS_GEMAN_MCCLURE); break;               \
    }

static bool loss_args_ok(int kind, float c) {
    return kind >= NR_LOSS_MSE && kind <= NR_LOSS_GEMAN_MCCLURE && std::isfinite(c) && c > 0.f;
}

int nr_robust_fwd_bwd(const float* pred, const float* target, int B, int kind, float c, float scale, float* loss2,
                      float* g, nr_stream_t stream) {
    NR_REQUIRE(pred && target && B > 0, "nr_robust_fwd_bwd: bad arguments");
    NR_REQUIRE(loss_args_ok(kind, c), "nr_robust_fwd_bwd: kind %d outside NR_LOSS_*, or c = %g not finite and > 0",
               kind, static_cast<double>(c));
#define NR_LAUNCH_ROBUST(KIND)                                                                                      \
    hipLaunchKernelGGL(robust_kernel<KIND>, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), pred, target, \
                       3 * B, c, scale, loss2, g)
    NR_LOSS_DISPATCH(kind, NR_LAUNCH_ROBUST)
#undef NR_LAUNCH_ROBUST
    NR_LAUNCH_CHECK("nr_robust_fwd_bwd");
    return NR_OK;
}

// The fused training launch.  rho_ray NULL: the MSE form (one loss word, kind and c unused);
// otherwise the loss family's (two loss words).  sqerr: B floats, then the long-ray seed's 3B.
static int composite_train(const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise,
                           const float* target, int B, int S, int white, int kind, float c, float scale,
                           float* rgb_map, float* depth, float* acc, float* weights, float* loss, float* g_rgb,
                           float* g_sigma, float* g_rd, unsigned* ticket, float* rho_ray, float* sqerr,
                           nr_stream_t stream) {
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const float inv = 1.0f / static_cast<float>(3 * B);
    const CompositeForm f = composite_form(B, S);
    // the in-launch loss sum pays up to ~256 workgroups; beyond, the agent-scope release and
    // ticket of every workgroup cost more than a second one-block launch (measured: 1024
    // workgroups, 4096 rays, 61 vs 26 + 5 us)
    if (ticket && ceil_div(B, 4) > 256) ticket = nullptr;
    if (f.wave) {
#define NR_LAUNCH_ROBUST(KIND)                                                                                     \
    hipLaunchKernelGGL(composite_robust_wave_kernel<KIND>, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, target, \
                       B, S, f.K, white, inv, scale, c, rgb_map, depth, acc, weights, sqerr, rho_ray, g_rgb,       \
                       g_sigma, g_rd, ticket, loss)
        if (rho_ray) {
            NR_LOSS_DISPATCH(kind, NR_LAUNCH_ROBUST)
        } else {
            hipLaunchKernelGGL(composite_mse_wave_kernel, f.grid, f.block, 0, s, rgb, sigma, z, rd, noise, target, B,
                               S, f.K, white, inv, scale, rgb_map, depth, acc, weights, sqerr, g_rgb, g_sigma, g_rd,
                               ticket, loss);
        }
#undef NR_LAUNCH_ROBUST
        NR_LAUNCH_CHECK(rho_ray ? "nr_composite_robust" : "nr_composite_mse");
        if (!ticket) {
            if (rho_ray) hipLaunchKernelGGL(loss2_sum_kernel, dim3(1), dim3(1024), 0, s, rho_ray, sqerr, B, inv, loss);
            else hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, s, sqerr, B, inv, loss);
            NR_LAUNCH_CHECK(rho_ray ? "nr_composite_robust (loss)" : "nr_composite_mse (loss)");
        }
        return NR_OK;
    }
    // long rays: the three separate passes (the seed gradient lives in the workspace)
    float* g_map = sqerr + B;
    int rc = nr_composite_fwd(rgb, sigma, z, rd, noise, B, S, white, rgb_map, depth, acc, weights, stream);
    if (rc) return rc;
    rc = rho_ray ? nr_robust_fwd_bwd(rgb_map, target, B, kind, c, scale, loss, g_map, stream)
                 : nr_mse_fwd_bwd(rgb_map, target, B, scale, loss, g_map, stream);
    if (rc) return rc;
    return nr_composite_bwd(rgb, sigma, z, rd, noise, B, S, white, g_map, nullptr, nullptr, nullptr, g_rgb, g_sigma,
                            g_rd, stream);
}

int64_t nr_composite_mse_workspace_bytes(int B) { return B > 0 ? int64_t{16} * B : 0; }

int nr_composite_mse(const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise,
                     const float* target, int B, int S, int white, float scale, float* rgb_map, float* depth,
                     float* acc, float* weights, float* loss, float* g_rgb, float* g_sigma, float* g_rd,
                     unsigned* ticket, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(rgb && sigma && z && rd && target && rgb_map && loss && g_rgb && g_sigma && workspace && B > 0 && S > 0,
               "nr_composite_mse: bad arguments");
    return composite_train(rgb, sigma, z, rd, noise, target, B, S, white, NR_LOSS_MSE, 0.f, scale, rgb_map, depth, acc,
                           weights, loss, g_rgb, g_sigma, g_rd, ticket, nullptr, static_cast<float*>(workspace),
                           stream);
}

// workspace: rho per ray (B), squared error per ray (B), the long-ray seed gradient (3B)
int64_t nr_composite_robust_workspace_bytes(int B) { return B > 0 ? int64_t{20} * B : 0; }

int nr_composite_robust(const float* rgb, const float* sigma, const float* z, const float* rd, const float* noise,
                        const float* target, int B, int S, int white, int kind, float c, float scale, float* rgb_map,
                        float* depth, float* acc, float* weights, float* loss2, float* g_rgb, float* g_sigma,
                        float* g_rd, unsigned* ticket, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(rgb && sigma && z && rd && target && rgb_map && loss2 && g_rgb && g_sigma && workspace && B > 0 && S > 0,
               "nr_composite_robust: bad arguments");
    NR_REQUIRE(loss_args_ok(kind, c), "nr_composite_robust: kind %d outside NR_LOSS_*, or c = %g not finite and > 0",
               kind, static_cast<double>(c));
    float* rho_ray = static_cast<float*>(workspace);
    return composite_train(rgb, sigma, z, rd, noise, target, B, S, white, kind, c, scale, rgb_map, depth, acc, weights,
                           loss2, g_rgb, g_sigma, g_rd, ticket, rho_ray, rho_ray + B, stream);
}

}  // extern "C"
