// Ray generation, SE(3) camera poses, stratified sampling and positional
// encoding: the per-ray / per-sample elementwise part of the hot path.
//
// Reference semantics (ShawnnnLiu/Robust-NeRF):
//   get_ray_directions  noisy_src/rays.py:17-64
//   get_rays            noisy_src/rays.py:67-99
//   get_rays_from_pixels noisy_src/data_pose_opt.py:83-148, :200-223
//   CameraPoseParameters noisy_src/train_pose_opt.py:122-226
//   sample_along_rays   noisy_src/rays.py:145-210
//   PositionalEncoding  noisy_src/model.py:20-80
// The library is built with -ffp-contract=off so that each a*b+c rounds twice,
// exactly as the reference's separate eager torch ops do.
//
// One body per computation: the learned-intrinsics entries (nr_*_xy, nr_*_intr_*, nr_*_lens*)
// and the windowed encoding run the kernels of the fixed-focal / plain entries (the focal pair
// as an argument or from device memory, the six-number lens from device memory, the window
// null or not), and every block reduction is block_sum_rows.  What the header promises to be bit-identical between two entries is so
// because both run the same code.
#include <type_traits>

#include "common.hpp"

namespace nr {

// torch.linspace(start, end, n)[i] (aten/native/cpu + cuda RangeFactories: symmetric form).
__device__ __forceinline__ float linspace_at(float start, float end, int n, int i) {
    if (n == 1) return start;
    const float step = (end - start) / static_cast<float>(n - 1);
    const int halfway = n / 2;
    return i < halfway ? start + step * static_cast<float>(i)
                       : end - step * static_cast<float>(n - 1 - i);
}

// ---------------------------------------------------------------- A1 -----
// Radial factor of the lens model (NeRF-- / SCNeRF form, on the ray side, so closed form):
// s = 1 + r2 (k1 + k2 r2) with r2 = x^2 + y^2 of the pinhole direction.  k1 == k2 == 0 gives
// exactly 1.0f for any finite r2, and x * 1.0f == x, so a lens without distortion leaves the
// pinhole direction's bits alone.
__device__ __forceinline__ float radial_scale(float x, float y, float k1, float k2, float& r2) {
    r2 = x * x + y * y;
    return 1.0f + r2 * (k1 + k2 * r2);
}

// A focal length per axis: the reference has one (nr_ray_directions passes it twice), learned
// intrinsics have two (nr_ray_directions_xy), a learned lens adds k1, k2 (nr_ray_directions_lens;
// the other two pass zeros).
__global__ void ray_directions_kernel(int H, int W, float fx, float fy, float cx, float cy, float k1, float k2,
                                      float* dirs) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const int j = p / W, i = p % W;  // meshgrid indexing='xy': dirs[j][i]
    const float xn = (static_cast<float>(i) - cx) / fx;
    const float yn = (static_cast<float>(j) - cy) / fy;
    float r2;
    const float s = radial_scale(xn, yn, k1, k2, r2);
    dirs[3 * p + 0] = xn * s;
    dirs[3 * p + 1] = -(yn * s);
    dirs[3 * p + 2] = -1.0f;
}

// rays_d = normalize(sum_k dir[k] * R[:,k]) (rays.py:89-94), rays_o = t.
__device__ __forceinline__ void rotate_normalize(const float* R /*4x4 row-major*/, float dx, float dy,
                                                 float dz, float& ox, float& oy, float& oz) {
    const float vx = (dx * R[0] + dy * R[1]) + dz * R[2];
    const float vy = (dx * R[4] + dy * R[5]) + dz * R[6];
    const float vz = (dx * R[8] + dy * R[9]) + dz * R[10];
    const float n = norm3(vx, vy, vz);
    ox = vx / n;
    oy = vy / n;
    oz = vz / n;
}

// ---------------------------------------------------------------- A2 -----
__global__ void get_rays_kernel(const float* dirs, const float* c2w, int64_t N, float* ro, float* rd) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= N) return;
    float x, y, z;
    rotate_normalize(c2w, dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2], x, y, z);
    rd[3 * p] = x;
    rd[3 * p + 1] = y;
    rd[3 * p + 2] = z;
    ro[3 * p] = c2w[3];
    ro[3 * p + 1] = c2w[7];
    ro[3 * p + 2] = c2w[11];
}

// A2 backward (rays.py:67-99 is differentiable w.r.t. c2w and the directions):
// rays_d = v/|v|, v = R d  ->  g_v = (g_d - u (u.g_d)) / |v|,  g_R += g_v d^T,
// g_d(dirs) = R^T g_v;  rays_o = t  ->  g_t += g_o.  The sum over the N rays is a
// fixed-shape two-pass reduction (kGrBlocks partials of 12, then one block).
constexpr int kGrBlocks = 256, kGrThreads = 256;

// The one fixed-order block sum of this file, over N rows at once: wave xor-butterfly
// 32 -> 1, lane 0 of each wave to LDS, one barrier for all rows, the waves added in index
// order from 0.f.  Thread e < N returns row e's total (the others 0.f).  Every thread of
// the T-wide block calls it, once per kernel.
template <int N, int T>
__device__ __forceinline__ float block_sum_rows(const float (&acc)[N]) {
    static_assert(T % 64 == 0 && N <= T, "whole waves, one thread per row");
    __shared__ float part[N][T / 64];
    for (int e = 0; e < N; ++e) {
        float v = acc[e];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) part[e][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < N)
        for (int w = 0; w < T / 64; ++w) t += part[threadIdx.x][w];
    return t;
}

// Cotangent gv of v = R d, given g = dL/d(rays_d) of this ray (rays_d = v/|v|).
__device__ __forceinline__ void dir_cotangent(const float* R, const float d3[3], const float* g, float gv[3]) {
    const float vx = (d3[0] * R[0] + d3[1] * R[1]) + d3[2] * R[2];
    const float vy = (d3[0] * R[4] + d3[1] * R[5]) + d3[2] * R[6];
    const float vz = (d3[0] * R[8] + d3[1] * R[9]) + d3[2] * R[10];
    const float n = norm3(vx, vy, vz);
    const float ux = vx / n, uy = vy / n, uz = vz / n;
    const float gx = g[0], gy = g[1], gz = g[2];
    const float dot = ux * gx + uy * gy + uz * gz;
    gv[0] = (gx - ux * dot) / n;
    gv[1] = (gy - uy * dot) / n;
    gv[2] = (gz - uz * dot) / n;
}

// Where entry e of a pose gradient's 12 sums [R row-major (9) | t (3)] sits in the 4x4.
__device__ __forceinline__ int pose_slot(int e) { return e < 9 ? 4 * (e / 3) + (e % 3) : 4 * (e - 9) + 3; }

__global__ void __launch_bounds__(kGrThreads)
get_rays_bwd_partial_kernel(const float* dirs, const float* c2w, int64_t N, const float* g_ro, const float* g_rd,
                            float* g_dirs, float* partials) {
    const float* R = c2w;
    float acc[12];
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * kGrThreads + threadIdx.x; p < N;
         p += static_cast<int64_t>(kGrBlocks) * kGrThreads) {
        if (g_ro)
            for (int r = 0; r < 3; ++r) acc[9 + r] += g_ro[3 * p + r];
        if (!g_rd) continue;
        const float d3[3] = {dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2]};
        float gv[3];
        dir_cotangent(R, d3, g_rd + 3 * p, gv);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) acc[3 * r + k] += gv[r] * d3[k];
        if (g_dirs)
            for (int k = 0; k < 3; ++k)
                g_dirs[3 * p + k] = (R[k] * gv[0] + R[4 + k] * gv[1]) + R[8 + k] * gv[2];
    }
    const float t = block_sum_rows<12, kGrThreads>(acc);
    if (threadIdx.x < 12) partials[blockIdx.x * 12 + threadIdx.x] = t;
}

__global__ void __launch_bounds__(kGrThreads) get_rays_bwd_final_kernel(const float* partials, float* g_c2w) {
    static_assert(kGrThreads == kGrBlocks, "one partial per thread");
    float acc[12];
    for (int e = 0; e < 12; ++e) acc[e] = partials[threadIdx.x * 12 + e];
    const float t = block_sum_rows<12, kGrThreads>(acc);
    if (threadIdx.x < 12) g_c2w[pose_slot(threadIdx.x)] += t;
}

// ---------------------------------------------------------------- A3 -----
// Pinhole camera-frame direction of pixel (u,v): the reference gathers it from the
// precomputed get_ray_directions table with .long() (truncating) indices.
__device__ __forceinline__ void pixel_dir(const float* pix, int b, float fx, float fy, float cx, float cy, float& dx,
                                          float& dy) {
    const int u = static_cast<int>(pix[2 * b]);
    const int v = static_cast<int>(pix[2 * b + 1]);
    dx = (static_cast<float>(u) - cx) / fx;
    dy = -((static_cast<float>(v) - cy) / fy);
}

// The pixel kernels take their camera as Focal = float, the reference's one number as a
// kernel argument (no memory read); Focal = const float*, learned intrinsics {fx, fy}; or
// Focal = LensPtr, a learned lens {fx, fy, cx, cy, k1, k2}.  The last two are in DEVICE memory,
// read when the kernel runs: a captured graph then sees the value of each replay, where an
// argument would be baked in at capture.  One body serves all three.  The first two have the
// principal point at (W/2, H/2) and no distortion step at all, so fx == fy == focal gives the
// same rays and pose gradients to the bit by construction; the lens at that principal point
// with k1 == k2 == 0 multiplies by s == 1.0f and gives them too.
struct LensPtr {
    const float* p;
};
struct Camera {
    float fx, fy, cx, cy, k1, k2;
};
__device__ __forceinline__ Camera camera_of(float focal, int W, int H) {
    return {focal, focal, static_cast<float>(W) * 0.5f, static_cast<float>(H) * 0.5f, 0.f, 0.f};
}
__device__ __forceinline__ Camera camera_of(const float* fxy, int W, int H) {
    return {fxy[0], fxy[1], static_cast<float>(W) * 0.5f, static_cast<float>(H) * 0.5f, 0.f, 0.f};
}
__device__ __forceinline__ Camera camera_of(LensPtr lens, int, int) {
    return {lens.p[0], lens.p[1], lens.p[2], lens.p[3], lens.p[4], lens.p[5]};
}

template <typename Focal>
__global__ void rays_from_pixels_fwd_kernel(const int64_t* img_idx, const float* pix, const float* poses,
                                            int n_img, int H, int W, Focal focal, int B, float* ro,
                                            float* rd, int* bad_index) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t img = img_idx[b];
    if (img < 0 || img >= n_img) {  // out-of-range image index: poison the ray, never read out of bounds
        for (int c = 0; c < 3; ++c) ro[3 * b + c] = rd[3 * b + c] = __builtin_nanf("");
        if (bad_index) *bad_index = 1;  // validating mode: the host wrapper raises IndexError
        return;
    }
    const float* P = poses + 16 * img;
    const Camera cam = camera_of(focal, W, H);
    float dx, dy;
    pixel_dir(pix, b, cam.fx, cam.fy, cam.cx, cam.cy, dx, dy);
    if constexpr (std::is_same<Focal, LensPtr>::value) {
        float r2;
        const float s = radial_scale(dx, dy, cam.k1, cam.k2, r2);
        dx *= s;
        dy *= s;
    }
    float x, y, z;
    rotate_normalize(P, dx, dy, -1.0f, x, y, z);
    rd[3 * b] = x;
    rd[3 * b + 1] = y;
    rd[3 * b + 2] = z;
    ro[3 * b] = P[3];
    ro[3 * b + 1] = P[7];
    ro[3 * b + 2] = P[11];
}

// Segmented reduction, one workgroup per image: every thread walks the batch with a
// fixed stride and sums its own rays of that image in batch order, then the block
// combines the per-thread sums in a fixed tree.  No atomics: the pose gradient is
// bit-identical from run to run (VERDICT r1 "non-deterministic reductions").
// Rows 0..11 are dL/d(pose), [R row-major (9) | t (3)], ADDED to g_poses[img].  With
// learned intrinsics two more rows go through the same tree (each row is reduced on its
// own, so the first 12 do not change): the image's focal terms {dL/dfx, dL/dfy}, WRITTEN
// to focal_part[img] (an image without rays in the batch: an exact 0).  They are gv taken
// back to the camera frame (g_d = R^T gv) times d(dx)/d(fx) = -dx/fx, d(dy)/d(fy) = -dy/fy.
// A learned lens carries six such rows {fx, fy, cx, cy, k1, k2} (18 in all) to lens_part[img]:
// with (px, py) the pinhole direction, d = (px s, py s, -1) and q = g_dx px + g_dy py the
// cotangent of s, dL/dk1 = q r2, dL/dk2 = q r2^2, and the cotangent of the pinhole direction
// is g_p = g_d s + 2 p q (k1 + 2 k2 r2); then dL/dfx = g_px (-px/fx) as above,
// dL/dcx = g_px (-1/fx), dL/dcy = g_py (1/fy) (py = -(v - cy)/fy).
constexpr int kPoseRedThreads = 256;

template <typename Focal>
__global__ void __launch_bounds__(kPoseRedThreads)
rays_from_pixels_bwd_kernel(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H, int W,
                            Focal focal, int B, const float* g_ro, const float* g_rd, float* g_poses,
                            float* focal_part) {
    constexpr bool kLens = std::is_same<Focal, LensPtr>::value;
    constexpr bool kFocalGrad = kLens || std::is_pointer<Focal>::value;
    constexpr int kCamRows = kLens ? 6 : (kFocalGrad ? 2 : 0);
    constexpr int kRows = 12 + kCamRows;
    const int img = blockIdx.x;
    const float* P = poses + 16 * static_cast<int64_t>(img);
    const Camera cam = camera_of(focal, W, H);
    float acc[kRows];
    for (int e = 0; e < kRows; ++e) acc[e] = 0.f;
    for (int b = threadIdx.x; b < B; b += kPoseRedThreads) {
        if (img_idx[b] != img) continue;
        for (int r = 0; r < 3; ++r) acc[9 + r] += g_ro[3 * b + r];
        if (!g_rd) continue;
        float d3[3] = {0.f, 0.f, -1.0f}, gv[3];
        pixel_dir(pix, b, cam.fx, cam.fy, cam.cx, cam.cy, d3[0], d3[1]);
        const float px = d3[0], py = d3[1];  // the pinhole direction
        float r2 = 0.f, s = 1.0f;
        if constexpr (kLens) {
            s = radial_scale(px, py, cam.k1, cam.k2, r2);
            d3[0] *= s;
            d3[1] *= s;
        }
        dir_cotangent(P, d3, g_rd + 3 * b, gv);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) acc[3 * r + k] += gv[r] * d3[k];
        if constexpr (kFocalGrad) {
            float g_px = (P[0] * gv[0] + P[4] * gv[1]) + P[8] * gv[2];
            float g_py = (P[1] * gv[0] + P[5] * gv[1]) + P[9] * gv[2];
            if constexpr (kLens) {
                const float q = g_px * px + g_py * py;
                const float g_r2 = q * (cam.k1 + (2.0f * cam.k2) * r2);
                acc[16] += q * r2;
                acc[17] += q * (r2 * r2);
                g_px = g_px * s + (2.0f * px) * g_r2;
                g_py = g_py * s + (2.0f * py) * g_r2;
                acc[14] += g_px * (-1.0f / cam.fx);
                acc[15] += g_py * (1.0f / cam.fy);
            }
            acc[12] += g_px * (-px / cam.fx);
            acc[13] += g_py * (-py / cam.fy);
        }
    }
    const float t = block_sum_rows<kRows, kPoseRedThreads>(acc);
    const int e = threadIdx.x;
    if (e < 12)
        g_poses[16 * static_cast<int64_t>(img) + pose_slot(e)] += t;
    else if (e < kRows)
        focal_part[kCamRows * static_cast<int64_t>(img) + (e - 12)] = t;
}

// Any image index outside [0, n_img) -> flag[0] = 1 (checked by the host wrapper).
__global__ void check_img_idx_kernel(const int64_t* img_idx, int B, int n_img, int* flag) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (img_idx[b] < 0 || img_idx[b] >= n_img)) flag[0] = 1;
}

// One workgroup: thread t sums the N-wide camera partials (N = 2 focal, 6 lens) of images
// t, t + 256, ... in that order, then the fixed tree over the threads.  Writes g_cam[0..N-1]
// (n_img == 0: zeros).
template <int N>
__global__ void __launch_bounds__(kPoseRedThreads)
focal_grad_final_kernel(const float* focal_part, int n_img, float* g_cam) {
    float s[N];
    for (int e = 0; e < N; ++e) s[e] = 0.f;
    for (int i = threadIdx.x; i < n_img; i += kPoseRedThreads)
        for (int e = 0; e < N; ++e) s[e] += focal_part[N * static_cast<int64_t>(i) + e];
    const float t = block_sum_rows<N, kPoseRedThreads>(s);
    if (threadIdx.x < N) g_cam[threadIdx.x] = t;
}

// ---------------------------------------------------------------- A4 -----
// Rodrigues with the reference's small-angle rule (train_pose_opt.py:136-163).
__device__ void rodrigues(const float w[3], float R[9], bool& small) {
    const float ang = norm3(w[0], w[1], w[2]);
    small = ang < 1e-6f;
    const float a = small ? 1.0f : ang;
    const float k0 = w[0] / a, k1 = w[1] / a, k2 = w[2] / a;
    // K = skew(axis); K2 = K @ K
    const float K[9] = {0.f, -k2, k1, k2, 0.f, -k0, -k1, k0, 0.f};
    float K2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            K2[3 * r + c] = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
    const float s = sinf(a), cc = 1.0f - cosf(a);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const float I = (r == c) ? 1.0f : 0.0f;
            R[3 * r + c] = small ? I : (I + s * K[3 * r + c]) + cc * K2[3 * r + c];
        }
}

__global__ void se3_poses_fwd_kernel(const float* init, const float* rot, const float* trans,
                                     const int64_t* indices, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t idx = indices ? indices[i] : i;
    const float* P = init + 16 * idx;
    float* O = out + 16 * i;
    float Rn[9];
    if (rot) {
        const float w[3] = {rot[3 * idx], rot[3 * idx + 1], rot[3 * idx + 2]};
        float Rd[9];
        bool small;
        rodrigues(w, Rd, small);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                Rn[3 * r + c] = (Rd[3 * r] * P[c] + Rd[3 * r + 1] * P[4 + c]) + Rd[3 * r + 2] * P[8 + c];
    } else {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rn[3 * r + c] = P[4 * r + c];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) O[4 * r + c] = Rn[3 * r + c];
        O[4 * r + 3] = trans ? P[4 * r + 3] + trans[3 * idx + r] : P[4 * r + 3];
    }
    O[12] = 0.f;
    O[13] = 0.f;
    O[14] = 0.f;
    O[15] = 1.f;
}

// dL/d(rot delta) of one output pose: G = dL/d(pose_out) (4x4), P = init pose, w = delta.
__device__ void se3_rot_grad(const float* P, const float w[3], const float* G, int fixed_small, float gw[3]) {
    // g_Rdelta = g_Rnew @ R_init^T
    float gRd[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            gRd[3 * r + c] = (G[4 * r] * P[4 * c] + G[4 * r + 1] * P[4 * c + 1]) + G[4 * r + 2] * P[4 * c + 2];
    const float th = norm3(w[0], w[1], w[2]);
    gw[0] = gw[1] = gw[2] = 0.f;
    // skew(e_m) entries: E_m[r][c]
    auto E = [](int m, int r, int c) -> float {
        // skew(v) = [[0,-v2,v1],[v2,0,-v0],[-v1,v0,0]]
        const int id = 3 * r + c;
        if (m == 0) return id == 5 ? -1.f : (id == 7 ? 1.f : 0.f);
        if (m == 1) return id == 2 ? 1.f : (id == 6 ? -1.f : 0.f);
        return id == 1 ? -1.f : (id == 3 ? 1.f : 0.f);
    };
    if (th < 1e-6f) {
        // Reference: torch.where(small, I, R) -> exactly zero gradient (train_pose_opt.py:143-161).
        if (fixed_small)
            for (int m = 0; m < 3; ++m) {
                float s = 0.f;
                for (int e = 0; e < 9; ++e) s += gRd[e] * E(m, e / 3, e % 3);
                gw[m] = s;
            }
    } else {
        const float a[3] = {w[0] / th, w[1] / th, w[2] / th};
        const float K[9] = {0.f, -a[2], a[1], a[2], 0.f, -a[0], -a[1], a[0], 0.f};
        float K2[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
        const float s = sinf(th), cs = cosf(th), cc = 1.f - cs;
        float g_th = 0.f;
        for (int e = 0; e < 9; ++e) g_th += gRd[e] * (cs * K[e] + s * K2[e]);
        float ga[3];
        for (int m = 0; m < 3; ++m) {
            float acc = 0.f;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    float EK = 0.f, KE = 0.f;
                    for (int q = 0; q < 3; ++q) {
                        EK += E(m, r, q) * K[3 * q + c];
                        KE += K[3 * r + q] * E(m, q, c);
                    }
                    acc += gRd[3 * r + c] * (s * E(m, r, c) + cc * (EK + KE));
                }
            ga[m] = acc;
        }
        const float adg = a[0] * ga[0] + a[1] * ga[1] + a[2] * ga[2];
        for (int m = 0; m < 3; ++m) gw[m] = g_th * a[m] + (ga[m] - a[m] * adg) / th;
    }
}

// One thread per pose p of the parameter table: sums the gradients of every output
// row i with indices[i] == p in row order (indices NULL: row p only).  Deterministic,
// no atomics, repeated indices allowed.
__global__ void se3_poses_bwd_kernel(const float* init, const float* rot, const int64_t* indices, int n,
                                     int n_poses, const float* g_poses, int fixed_small, float* g_rot,
                                     float* g_trans) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_poses) return;
    const float* P = init + 16 * static_cast<int64_t>(p);
    const bool want_rot = g_rot && rot;
    const float w[3] = {want_rot ? rot[3 * p] : 0.f, want_rot ? rot[3 * p + 1] : 0.f, want_rot ? rot[3 * p + 2] : 0.f};
    float st[3] = {0.f, 0.f, 0.f}, sr[3] = {0.f, 0.f, 0.f};
    const int i0 = indices ? 0 : p, i1 = indices ? n : (p < n ? p + 1 : p);
    for (int i = i0; i < i1; ++i) {
        if (indices && indices[i] != p) continue;
        const float* G = g_poses + 16 * static_cast<int64_t>(i);
        for (int r = 0; r < 3; ++r) st[r] += G[4 * r + 3];
        if (want_rot) {
            float gw[3];
            se3_rot_grad(P, w, G, fixed_small, gw);
            for (int m = 0; m < 3; ++m) sr[m] += gw[m];
        }
    }
    if (g_trans)
        for (int r = 0; r < 3; ++r) g_trans[3 * p + r] += st[r];
    if (want_rot)
        for (int m = 0; m < 3; ++m) g_rot[3 * p + m] += sr[m];
}

// ------------------------------------------------ batch assembly (§8f-1) -
// RaySampler (data.py:264-321): rows idx[b] of the device ray table (rays_o,
// rays_d, colors; 36 B per ray) into one batch, one launch for all three.
__global__ void gather_rays_kernel(const int64_t* idx, int64_t n_rays, int B, const float* ro, const float* rd,
                                   const float* rgb, float* out_o, float* out_d, float* out_rgb,
                                   int* bad_index) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t i = idx[b];
    const bool ok = i >= 0 && i < n_rays;
    if (!ok && bad_index) *bad_index = 1;  // validating mode: the host wrapper raises IndexError
    for (int c = 0; c < 3; ++c) {
        out_o[3 * b + c] = ok ? ro[3 * i + c] : __builtin_nanf("");
        out_d[3 * b + c] = ok ? rd[3 * i + c] : __builtin_nanf("");
        out_rgb[3 * b + c] = ok ? rgb[3 * i + c] : __builtin_nanf("");
    }
}

// PixelSampler.sample_batch (data_pose_opt.py:178-198): flat pixel index ->
// (image, (u, v), colour).  The reference's image_indices / pixel_coords tables
// are pure functions of the index, so only the images are read.  64-bit index
// arithmetic throughout: n_img * H * W may exceed 2^31.
__global__ void gather_pixels_kernel(const int64_t* idx, int64_t n_pixels, int64_t hw, int64_t W, const float* images,
                                     int B, int64_t* out_img, float* out_pix, float* out_rgb, int* bad_index) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t i = idx[b];
    const bool ok = i >= 0 && i < n_pixels;
    if (!ok && bad_index) *bad_index = 1;  // validating mode: the host wrapper raises IndexError
    const float nan = __builtin_nanf("");
    out_img[b] = ok ? i / hw : -1;
    out_pix[2 * b + 0] = ok ? static_cast<float>(i % W) : nan;         // u (hw is a multiple of W)
    out_pix[2 * b + 1] = ok ? static_cast<float>((i % hw) / W) : nan;  // v
    for (int c = 0; c < 3; ++c) out_rgb[3 * b + c] = ok ? images[3 * i + c] : nan;
}

// ---------------------------------------------------------------- A5 -----
__global__ void stratified_kernel(const float* ro, const float* rd, const float* t_rand, float near_,
                                  float far_, int lindisp, int B, int N, float* z_out, float* pts, float* vd) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= static_cast<int64_t>(B) * N) return;
    const int b = static_cast<int>(p / N), i = static_cast<int>(p % N);
    auto zlin = [&](int k) -> float {
        const float t = linspace_at(0.f, 1.f, N, k);
        if (lindisp) return 1.0f / ((1.0f / near_) * (1.0f - t) + (1.0f / far_) * t);
        return near_ * (1.0f - t) + far_ * t;
    };
    float z = zlin(i);
    if (t_rand) {
        const float zp = i > 0 ? zlin(i - 1) : 0.f;
        const float zn = i < N - 1 ? zlin(i + 1) : 0.f;
        const float lower = i > 0 ? 0.5f * (z + zp) : z;      // cat([z[:1], mids])
        const float upper = i < N - 1 ? 0.5f * (zn + z) : z;  // cat([mids, z[-1:]])
        z = lower + (upper - lower) * t_rand[p];
    }
    z_out[p] = z;
    if (pts) {
        for (int c = 0; c < 3; ++c) pts[3 * p + c] = ro[3 * b + c] + rd[3 * b + c] * z;
    }
    if (vd) {  // rendering.py:165, broadcast to the samples (expand_viewdirs_kernel's values)
        const float x = rd[3 * b], y = rd[3 * b + 1], w = rd[3 * b + 2];
        const float n = norm3(x, y, w);
        vd[3 * p] = x / n;
        vd[3 * p + 1] = y / n;
        vd[3 * p + 2] = w / n;
    }
}

// ---------------------------------------------------------------- A6 -----
__device__ __forceinline__ float pe_freq(int k, int L, int log_sampling) {
    if (log_sampling) return exp2f(linspace_at(0.f, static_cast<float>(L - 1), L, k));
    return linspace_at(1.f, exp2f(static_cast<float>(L - 1)), L, k);
}

// The encoding, plain (w null: the reference's) or windowed for coarse-to-fine registration:
// frequency k's sin and cos times w[k], read from device memory; the raw input block is not
// weighted.  In the backward a null w multiplies by 1.0f, which is exact.
__global__ void pe_kernel(const float* x, int64_t M, int C, int L, int inc, int logs, const float* w, float* out) {
    const int D = inc + 2 * L;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= M * C * D) return;
    const int64_t m = p / (C * D);
    const int col = static_cast<int>(p % (C * D));
    const int blk = col / C, c = col % C;  // output block blk of width C
    const float v = x[m * C + c];
    float r;
    if (inc && blk == 0) {
        r = v;
    } else {
        const int q = blk - inc;
        const float f = pe_freq(q >> 1, L, logs);
        r = (q & 1) ? cosf(f * v) : sinf(f * v);
        if (w) r *= w[q >> 1];
    }
    out[p] = r;
}

__global__ void pe_bwd_kernel(const float* x, int64_t M, int C, int L, int inc, int logs, const float* w,
                              const float* g, float* gx) {
    const int D = inc + 2 * L;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= M * C) return;
    const int64_t m = p / C;
    const int c = static_cast<int>(p % C);
    const float v = x[p];
    const float* gr = g + m * C * D;
    float acc = inc ? gr[c] : 0.f;
    for (int k = 0; k < L; ++k) {
        const float f = pe_freq(k, L, logs);
        const float a = f * v;
        const float wk = w ? w[k] : 1.0f;
        acc += wk * (gr[(inc + 2 * k) * C + c] * (cosf(a) * f));
        acc += wk * (gr[(inc + 2 * k + 1) * C + c] * (-sinf(a) * f));
    }
    gx[p] = acc;
}

// ---------------------------------------------------------------- glue ----
__global__ void expand_viewdirs_kernel(const float* rd, int B, int S, float* out) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= static_cast<int64_t>(B) * S) return;
    const int b = static_cast<int>(p / S);
    const float x = rd[3 * b], y = rd[3 * b + 1], z = rd[3 * b + 2];
    const float n = norm3(x, y, z);
    out[3 * p] = x / n;
    out[3 * p + 1] = y / n;
    out[3 * p + 2] = z / n;
}

// One wave per ray: sum over its S samples.
__global__ void pts_bwd_kernel(const float* g_pts, const float* z, int B, int S, float* g_ro, float* g_rd) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
    for (int s = lane; s < S; s += 64) {
        const int64_t q = static_cast<int64_t>(b) * S + s;
        const float zz = z[q];
        for (int c = 0; c < 3; ++c) {
            const float g = g_pts[3 * q + c];
            so[c] += g;
            sd[c] += g * zz;
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int c = 0; c < 3; ++c) {
            so[c] += __shfl_xor(so[c], off);
            sd[c] += __shfl_xor(sd[c], off);
        }
    if (lane == 0)
        for (int c = 0; c < 3; ++c) {
            if (g_ro) g_ro[3 * b + c] += so[c];
            if (g_rd) g_rd[3 * b + c] += sd[c];
        }
}

__global__ void viewdirs_bwd_kernel(const float* rd, const float* g_vd, int B, int S, float* g_rd) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    float sg[3] = {0.f, 0.f, 0.f};
    for (int s = lane; s < S; s += 64) {
        const int64_t q = static_cast<int64_t>(b) * S + s;
        for (int c = 0; c < 3; ++c) sg[c] += g_vd[3 * q + c];
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int c = 0; c < 3; ++c) sg[c] += __shfl_xor(sg[c], off);
    if (lane == 0) {
        const float x = rd[3 * b], y = rd[3 * b + 1], z = rd[3 * b + 2];
        const float n = norm3(x, y, z);
        const float u[3] = {x / n, y / n, z / n};
        const float dot = u[0] * sg[0] + u[1] * sg[1] + u[2] * sg[2];
        for (int c = 0; c < 3; ++c) g_rd[3 * b + c] += (sg[c] - u[c] * dot) / n;
    }
}

}  // namespace nr

using namespace nr;

extern "C" {

int nr_ray_directions(int H, int W, float focal, float cx, float cy, float* dirs, nr_stream_t stream) {
    NR_REQUIRE(H > 0 && W > 0 && dirs, "nr_ray_directions: bad arguments");
    const int n = H * W;
    hipLaunchKernelGGL(ray_directions_kernel, dim3(ceil_div(n, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), H, W, focal, focal, cx, cy, 0.f, 0.f, dirs);
    NR_LAUNCH_CHECK("nr_ray_directions");
    return NR_OK;
}

int nr_ray_directions_xy(int H, int W, float fx, float fy, float cx, float cy, float* dirs, nr_stream_t stream) {
    NR_REQUIRE(H > 0 && W > 0 && dirs, "nr_ray_directions_xy: bad arguments");
    const int n = H * W;
    hipLaunchKernelGGL(ray_directions_kernel, dim3(ceil_div(n, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), H, W, fx, fy, cx, cy, 0.f, 0.f, dirs);
    NR_LAUNCH_CHECK("nr_ray_directions_xy");
    return NR_OK;
}

int nr_ray_directions_lens(int H, int W, float fx, float fy, float cx, float cy, float k1, float k2, float* dirs,
                           nr_stream_t stream) {
    NR_REQUIRE(H > 0 && W > 0 && dirs, "nr_ray_directions_lens: bad arguments");
    const int n = H * W;
    hipLaunchKernelGGL(ray_directions_kernel, dim3(ceil_div(n, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), H, W, fx, fy, cx, cy, k1, k2, dirs);
    NR_LAUNCH_CHECK("nr_ray_directions_lens");
    return NR_OK;
}

int nr_get_rays(const float* dirs, const float* c2w, int64_t N, float* ro, float* rd, nr_stream_t stream) {
    NR_REQUIRE(dirs && c2w && ro && rd && N >= 0, "nr_get_rays: bad arguments");
    if (N == 0) return NR_OK;
    hipLaunchKernelGGL(get_rays_kernel, dim3(static_cast<unsigned>(ceil_div_ll(N, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dirs, c2w, N, ro, rd);
    NR_LAUNCH_CHECK("nr_get_rays");
    return NR_OK;
}

int64_t nr_get_rays_bwd_workspace_bytes(void) { return static_cast<int64_t>(kGrBlocks) * 12 * sizeof(float); }

int nr_get_rays_bwd(const float* dirs, const float* c2w, int64_t N, const float* g_ro, const float* g_rd,
                    float* g_dirs, float* g_c2w, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(dirs && c2w && g_c2w && workspace && N >= 0 && (g_ro || g_rd) && (!g_dirs || g_rd),
               "nr_get_rays_bwd: bad arguments");
    if (N == 0) return NR_OK;
    float* partials = static_cast<float*>(workspace);
    hipLaunchKernelGGL(get_rays_bwd_partial_kernel, dim3(kGrBlocks), dim3(kGrThreads), 0,
                       static_cast<hipStream_t>(stream), dirs, c2w, N, g_ro, g_rd, g_dirs, partials);
    NR_LAUNCH_CHECK("nr_get_rays_bwd");
    hipLaunchKernelGGL(get_rays_bwd_final_kernel, dim3(1), dim3(kGrThreads), 0, static_cast<hipStream_t>(stream),
                       partials, g_c2w);
    NR_LAUNCH_CHECK("nr_get_rays_bwd");
    return NR_OK;
}

int nr_rays_from_pixels_fwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                            int W, float focal, int B, float* ro, float* rd, int* bad_index,
                            nr_stream_t stream) {
    NR_REQUIRE(img_idx && pix && poses && ro && rd && B >= 0 && n_img > 0, "nr_rays_from_pixels_fwd: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(rays_from_pixels_fwd_kernel<float>, dim3(ceil_div(B, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, focal, B, ro, rd,
                       bad_index);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_fwd");
    return NR_OK;
}

int nr_rays_from_pixels_bwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                            int W, float focal, int B, const float* g_ro, const float* g_rd, float* g_poses,
                            nr_stream_t stream) {
    NR_REQUIRE(img_idx && pix && poses && g_ro && g_poses && B >= 0 && n_img > 0,
               "nr_rays_from_pixels_bwd: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(rays_from_pixels_bwd_kernel<float>, dim3(n_img), dim3(kPoseRedThreads), 0,
                       static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, focal, B, g_ro, g_rd,
                       g_poses, nullptr);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_bwd");
    return NR_OK;
}

int nr_rays_from_pixels_intr_fwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                                 int W, const float* fxy, int B, float* ro, float* rd, int* bad_index,
                                 nr_stream_t stream) {
    // an empty batch may come with null arrays (a zero-size tensor has no storage)
    NR_REQUIRE(fxy && B >= 0 && n_img > 0 && (B == 0 || (img_idx && pix && poses && ro && rd)),
               "nr_rays_from_pixels_intr_fwd: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(rays_from_pixels_fwd_kernel<const float*>, dim3(ceil_div(B, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, fxy, B, ro, rd,
                       bad_index);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_intr_fwd");
    return NR_OK;
}

int64_t nr_rays_from_pixels_intr_bwd_workspace_bytes(int n_img) {
    return static_cast<int64_t>(n_img > 0 ? n_img : 1) * 2 * sizeof(float);
}

int nr_rays_from_pixels_intr_bwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                                 int W, const float* fxy, int B, const float* g_ro, const float* g_rd,
                                 float* g_poses, float* g_fxy, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(fxy && g_poses && g_fxy && workspace && B >= 0 && n_img > 0 &&
                   (B == 0 || (img_idx && pix && poses && g_ro)),
               "nr_rays_from_pixels_intr_bwd: bad arguments");
    float* focal_part = static_cast<float*>(workspace);
    if (B > 0) {
        hipLaunchKernelGGL(rays_from_pixels_bwd_kernel<const float*>, dim3(n_img), dim3(kPoseRedThreads), 0,
                           static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, fxy, B, g_ro, g_rd,
                           g_poses, focal_part);
        NR_LAUNCH_CHECK("nr_rays_from_pixels_intr_bwd");
    }
    // an empty batch has no partials: the final launch then writes zeros
    hipLaunchKernelGGL(focal_grad_final_kernel<2>, dim3(1), dim3(kPoseRedThreads), 0,
                       static_cast<hipStream_t>(stream), focal_part, B > 0 ? n_img : 0, g_fxy);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_intr_bwd");
    return NR_OK;
}

int nr_rays_from_pixels_lens_fwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                                 int W, const float* lens, int B, float* ro, float* rd, int* bad_index,
                                 nr_stream_t stream) {
    NR_REQUIRE(lens && B >= 0 && n_img > 0 && (B == 0 || (img_idx && pix && poses && ro && rd)),
               "nr_rays_from_pixels_lens_fwd: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(rays_from_pixels_fwd_kernel<LensPtr>, dim3(ceil_div(B, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, LensPtr{lens}, B, ro, rd,
                       bad_index);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_lens_fwd");
    return NR_OK;
}

int64_t nr_rays_from_pixels_lens_bwd_workspace_bytes(int n_img) {
    return static_cast<int64_t>(n_img > 0 ? n_img : 1) * 6 * sizeof(float);
}

int nr_rays_from_pixels_lens_bwd(const int64_t* img_idx, const float* pix, const float* poses, int n_img, int H,
                                 int W, const float* lens, int B, const float* g_ro, const float* g_rd,
                                 float* g_poses, float* g_lens, void* workspace, nr_stream_t stream) {
    NR_REQUIRE(lens && g_poses && g_lens && workspace && B >= 0 && n_img > 0 &&
                   (B == 0 || (img_idx && pix && poses && g_ro)),
               "nr_rays_from_pixels_lens_bwd: bad arguments");
    float* lens_part = static_cast<float*>(workspace);
    if (B > 0) {
        hipLaunchKernelGGL(rays_from_pixels_bwd_kernel<LensPtr>, dim3(n_img), dim3(kPoseRedThreads), 0,
                           static_cast<hipStream_t>(stream), img_idx, pix, poses, n_img, H, W, LensPtr{lens}, B, g_ro,
                           g_rd, g_poses, lens_part);
        NR_LAUNCH_CHECK("nr_rays_from_pixels_lens_bwd");
    }
    // an empty batch has no partials: the final launch then writes zeros
    hipLaunchKernelGGL(focal_grad_final_kernel<6>, dim3(1), dim3(kPoseRedThreads), 0,
                       static_cast<hipStream_t>(stream), lens_part, B > 0 ? n_img : 0, g_lens);
    NR_LAUNCH_CHECK("nr_rays_from_pixels_lens_bwd");
    return NR_OK;
}

int nr_check_index_range(const int64_t* idx, int n, int limit, int* flag, nr_stream_t stream) {
    NR_REQUIRE(idx && flag && n >= 0 && limit >= 0, "nr_check_index_range: bad arguments");
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(check_img_idx_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       idx, n, limit, flag);
    NR_LAUNCH_CHECK("nr_check_index_range");
    return NR_OK;
}

int nr_se3_poses_fwd(const float* init, const float* rot, const float* trans, const int64_t* indices, int n,
                     float* out, nr_stream_t stream) {
    NR_REQUIRE(init && out && n >= 0, "nr_se3_poses_fwd: bad arguments");
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(se3_poses_fwd_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       init, rot, trans, indices, n, out);
    NR_LAUNCH_CHECK("nr_se3_poses_fwd");
    return NR_OK;
}

int nr_se3_poses_bwd(const float* init, const float* rot, const int64_t* indices, int n, int n_poses,
                     const float* g_poses, int fixed_small, float* g_rot, float* g_trans, nr_stream_t stream) {
    NR_REQUIRE(init && g_poses && n >= 0 && n_poses >= 0 && (indices || n <= n_poses),
               "nr_se3_poses_bwd: bad arguments");
    if (n == 0 || n_poses == 0) return NR_OK;
    hipLaunchKernelGGL(se3_poses_bwd_kernel, dim3(ceil_div(n_poses, 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), init, rot, indices, n, n_poses, g_poses, fixed_small, g_rot,
                       g_trans);
    NR_LAUNCH_CHECK("nr_se3_poses_bwd");
    return NR_OK;
}

int nr_gather_rays(const int64_t* idx, int64_t n_rays, int B, const float* rays_o, const float* rays_d,
                   const float* colors, float* out_o, float* out_d, float* out_rgb, int* bad_index,
                   nr_stream_t stream) {
    NR_REQUIRE(idx && rays_o && rays_d && colors && out_o && out_d && out_rgb && B >= 0 && n_rays >= 0,
               "nr_gather_rays: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(gather_rays_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), idx,
                       n_rays, B, rays_o, rays_d, colors, out_o, out_d, out_rgb, bad_index);
    NR_LAUNCH_CHECK("nr_gather_rays");
    return NR_OK;
}

int nr_gather_pixels(const int64_t* idx, int n_img, int H, int W, const float* images, int B, int64_t* out_img,
                     float* out_pix, float* out_rgb, int* bad_index, nr_stream_t stream) {
    NR_REQUIRE(idx && images && out_img && out_pix && out_rgb && B >= 0 && n_img >= 0 && H > 0 && W > 0,
               "nr_gather_pixels: bad arguments");
    if (B == 0) return NR_OK;
    const int64_t hw = static_cast<int64_t>(H) * W;
    hipLaunchKernelGGL(gather_pixels_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), idx,
                       n_img * hw, hw, static_cast<int64_t>(W), images, B, out_img, out_pix, out_rgb, bad_index);
    NR_LAUNCH_CHECK("nr_gather_pixels");
    return NR_OK;
}

int nr_stratified_sample(const float* ro, const float* rd, const float* t_rand, float near_, float far_,
                         int lindisp, int B, int N, float* z, float* pts, float* viewdirs, nr_stream_t stream) {
    NR_REQUIRE(z && B >= 0 && N > 0 && (!pts || (ro && rd)) && (!viewdirs || rd),
               "nr_stratified_sample: bad arguments");
    const int64_t n = static_cast<int64_t>(B) * N;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(stratified_kernel, dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), ro, rd, t_rand, near_, far_, lindisp, B, N, z, pts, viewdirs);
    NR_LAUNCH_CHECK("nr_stratified_sample");
    return NR_OK;
}

int nr_positional_encoding(const float* x, int64_t M, int C, int L, int inc, int logs, float* out,
                           nr_stream_t stream) {
    NR_REQUIRE(x && out && M >= 0 && C > 0 && L >= 0, "nr_positional_encoding: bad arguments");
    const int64_t n = M * C * (inc + 2 * L);
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(pe_kernel, dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, M, C, L, inc, logs, nullptr, out);
    NR_LAUNCH_CHECK("nr_positional_encoding");
    return NR_OK;
}

int nr_positional_encoding_bwd(const float* x, int64_t M, int C, int L, int inc, int logs, const float* g,
                               float* gx, nr_stream_t stream) {
    NR_REQUIRE(x && g && gx && M >= 0 && C > 0 && L >= 0, "nr_positional_encoding_bwd: bad arguments");
    const int64_t n = M * C;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(pe_bwd_kernel, dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, M, C, L, inc, logs, nullptr, g, gx);
    NR_LAUNCH_CHECK("nr_positional_encoding_bwd");
    return NR_OK;
}

int nr_positional_encoding_windowed(const float* x, int64_t M, int C, int L, int inc, int logs, const float* w,
                                    float* out, nr_stream_t stream) {
    NR_REQUIRE(x && out && M >= 0 && C > 0 && L >= 0, "nr_positional_encoding_windowed: bad arguments");
    const int64_t n = M * C * (inc + 2 * L);
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(pe_kernel,dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, M, C, L, inc, logs, w, out);
    NR_LAUNCH_CHECK("nr_positional_encoding_windowed");
    return NR_OK;
}

int nr_positional_encoding_windowed_bwd(const float* x, int64_t M, int C, int L, int inc, int logs, const float* w,
                                        const float* g, float* gx, nr_stream_t stream) {
    NR_REQUIRE(x && g && gx && M >= 0 && C > 0 && L >= 0, "nr_positional_encoding_windowed_bwd: bad arguments");
    const int64_t n = M * C;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(pe_bwd_kernel,dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, M, C, L, inc, logs, w, g, gx);
    NR_LAUNCH_CHECK("nr_positional_encoding_windowed_bwd");
    return NR_OK;
}

int nr_expand_viewdirs(const float* rd, int B, int S, float* out, nr_stream_t stream) {
    NR_REQUIRE(rd && out && B >= 0 && S > 0, "nr_expand_viewdirs: bad arguments");
    const int64_t n = static_cast<int64_t>(B) * S;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(expand_viewdirs_kernel, dim3(static_cast<unsigned>(ceil_div_ll(n, 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rd, B, S, out);
    NR_LAUNCH_CHECK("nr_expand_viewdirs");
    return NR_OK;
}

int nr_pts_bwd(const float* g_pts, const float* z, int B, int S, float* g_ro, float* g_rd, nr_stream_t stream) {
    NR_REQUIRE(g_pts && z && B >= 0 && S > 0, "nr_pts_bwd: bad arguments");
    if (B == 0 || (!g_ro && !g_rd)) return NR_OK;
    hipLaunchKernelGGL(pts_bwd_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), g_pts,
                       z, B, S, g_ro, g_rd);
    NR_LAUNCH_CHECK("nr_pts_bwd");
    return NR_OK;
}

int nr_viewdirs_bwd(const float* rd, const float* g_vd, int B, int S, float* g_rd, nr_stream_t stream) {
    NR_REQUIRE(rd && g_vd && g_rd && B >= 0 && S > 0, "nr_viewdirs_bwd: bad arguments");
    if (B == 0) return NR_OK;
    hipLaunchKernelGGL(viewdirs_bwd_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       rd, g_vd, B, S, g_rd);
    NR_LAUNCH_CHECK("nr_viewdirs_bwd");
    return NR_OK;
}

}  // extern "C"
