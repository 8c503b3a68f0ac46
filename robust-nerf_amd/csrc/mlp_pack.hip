// Weight packing of the fused NeRF MLP (the MFMA fragment images of mlp_plan.hpp, all
// precisions), the fused optimizer step that refreshes them in place, and the
// positional-encoding window folded into their encoding columns.
#include <cstring>

#include "mlp_dev.hpp"
#include "mlp_launch.hpp"

namespace nr {

// ---------------------------------------------------------------- pack ----
// Every pack kernel has an index mode (IDX): instead of writing a parameter's value
// into an image it records where it goes, in the destination table of the fused
// optimizer step (nr_adam_multi): table[slot * n + i] = kind << 29 | byte offset
// for flat parameter i.  Slot 0: the forward W image, a bias fragment or a pair
// image; 1: the W^T image or a vector image; 2: the 16-bit dX-chain image.  The
// same index maps fill both, so a refresh through the table writes exactly the
// bytes nr_mlp_pack writes.
// (kPackSlots, kDstMaxOff and PackIdx: mlp_launch.hpp)
enum : uint32_t { kDstNone = 0, kDstF32 = 1, kDstBf16 = 2, kDstF16 = 3, kDstFragBf16 = 4, kDstFragF16 = 5 };
__device__ __forceinline__ void put_dst(const PackIdx& t, int slot, int64_t pidx, int64_t off, uint32_t kind) {
    t.table[slot * t.n + pidx] = (kind << 29) | static_cast<uint32_t>(off);
}
__device__ __forceinline__ uint32_t dst16(int prec) { return prec == NR_PREC_FP16 ? kDstF16 : kDstBf16; }

// Image element e of layer l (fwd: W, bwd: W^T), chunk-major:
//   e = (((kblock * ROWBLOCKS + rowblock) * FPB + frag) * 64 + lane) * EPL + el
struct PackArgs {
    const float* params;
    char* packed;
    int n_lin;
    int prec;
    int64_t w_off[kMaxMfmaLayers];
    int in[kMaxMfmaLayers], NB[kMaxMfmaLayers], KB[kMaxMfmaLayers], nseg[kMaxMfmaLayers];
    int seg_col0[kMaxMfmaLayers][kMaxSeg], seg_w[kMaxMfmaLayers][kMaxSeg], seg_blk[kMaxMfmaLayers][kMaxSeg];
    int64_t pk[kMaxMfmaLayers], pkb[kMaxMfmaLayers];
    int bwd_rot[kMaxMfmaLayers];  // W^T row-block rotation: skip layers put the h rows first
    int64_t cum[kMaxMfmaLayers + 1];
};

// W column of local input index c (0..31) in input block kb, or -1 for padding.
__device__ __forceinline__ int pack_col(const PackArgs& a, int l, int kb, int c) {
    int blk0 = 0;
    for (int s = 0; s < a.nseg[l]; ++s) {
        if (kb < blk0 + a.seg_blk[l][s]) {
            const int cs = 32 * (kb - blk0) + c;
            return cs < a.seg_w[l][s] ? a.seg_col0[l][s] + cs : -1;
        }
        blk0 += a.seg_blk[l][s];
    }
    return -1;
}

// Image element e of layer l's W (bwd: W^T) image in pack order: the W entry it holds
// (col < 0: padding) and the element of the image it is stored at.
struct PackLoc {
    int row, col;
    int64_t dst_e;
};
__device__ __forceinline__ PackLoc pack_locate(const PackArgs& a, int l, int64_t e, bool bwd) {
    const bool bf = a.prec != NR_PREC_FP32;  // 16-bit image (bf16 or fp16)
    const int epl = bf ? 8 : 4, fpb = bf ? 2 : 4;
    const int64_t frag = e / (64 * epl);
    const int lane = static_cast<int>((e / epl) % 64);
    const int el = static_cast<int>(e % epl);
    const int64_t blk = frag / fpb;
    const int sub = static_cast<int>(frag % fpb);
    const int h = lane >> 5, i = lane & 31;
    const int kk = bf ? 16 * sub + 8 * (el >> 2) + 4 * h + (el & 3) : acc_row(4 * sub + el, h);
    PackLoc o;
    o.dst_e = e;
    if (!bwd) {  // W: A[i][k] = W[32nb + i][col(kb, k)]
        // fp32: chunk kb, row block nb (chunk-major); 16-bit: row block nb, k block kb,
        // then the row block's bias fragment (row-block major, mlp_fwd_rbm.inc)
        const int kb = static_cast<int>(bf ? blk % a.KB[l] : blk / a.NB[l]);
        const int nb = static_cast<int>(bf ? blk / a.KB[l] : blk % a.NB[l]);
        o.row = 32 * nb + i;
        o.col = pack_col(a, l, kb, kk);
        if (bf) o.dst_e = ((static_cast<int64_t>(nb) * (2 * a.KB[l] + 1) + 2 * kb + sub) * 64 + lane) * epl + el;
    } else {  // W^T: A[i][k] = W[32ob + k][col(ib, i)], chunk ob, row block ib
        const int ob = static_cast<int>(blk / a.KB[l]);
        const int ib = static_cast<int>((blk % a.KB[l] + a.bwd_rot[l]) % a.KB[l]);
        o.row = 32 * ob + kk;
        o.col = pack_col(a, l, ib, i);
    }
    return o;
}

// v, converted to the image's precision, into element dst_e of layer l's W (bwd: W^T) image
__device__ __forceinline__ void pack_store(const PackArgs& a, int l, bool bwd, int64_t dst_e, float v) {
    char* dst = a.packed + (bwd ? a.pkb[l] : a.pk[l]);
    if (a.prec != NR_PREC_FP32)
        reinterpret_cast<unsigned short*>(dst)[dst_e] =
            a.prec == NR_PREC_FP16 ? __builtin_bit_cast(unsigned short, static_cast<_Float16>(v)) : bf16_bits(v);
    else
        reinterpret_cast<float*>(dst)[dst_e] = v;
}

template <bool IDX>
__global__ void mlp_pack_kernel(PackArgs a, PackIdx t) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= a.cum[a.n_lin]) return;
    int l = 0;
    while (g >= a.cum[l + 1]) ++l;
    const int64_t img = (a.cum[l + 1] - a.cum[l]) / 2;
    int64_t e = g - a.cum[l];
    const bool bwd = e >= img;
    if (bwd) e -= img;
    const bool bf = a.prec != NR_PREC_FP32;
    const PackLoc o = pack_locate(a, l, e, bwd);
    if constexpr (IDX) {
        if (o.col >= 0)
            put_dst(t, bwd ? 1 : 0, a.w_off[l] + static_cast<int64_t>(o.row) * a.in[l] + o.col,
                    (bwd ? a.pkb[l] : a.pk[l]) + o.dst_e * (bf ? 2 : 4), bf ? dst16(a.prec) : kDstF32);
        return;
    }
    pack_store(a, l, bwd, o.dst_e,
               o.col >= 0 ? a.params[a.w_off[l] + static_cast<int64_t>(o.row) * a.in[l] + o.col] : 0.f);
}

// ------------------------------------------------ positional-encoding window ----
// A per-frequency weight w_k on an encoder's sin / cos columns (coarse-to-fine
// registration) is folded into the weights that read them: W . (s * gamma) = (W * s) . gamma
// with s = 1 on the 3 raw columns and w[(c - 3) / 6] on encoding column c.  The forward
// and the input gradients read W only through the images, so the MLP kernels run
// unchanged on folded images; their dW is dL/d(W * s), which window_grad_kernel scales
// by s into dL/dW.  A window pointer may be null: all ones.
__device__ __forceinline__ float window_scale(const float* w, int c) { return (w && c >= 3) ? w[(c - 3) / 6] : 1.0f; }

// The encoding segments of the plan: layer 0 and the layer after each skip (x_enc,
// which = 0), dir_linear (d_enc, which = 1).
struct WindowArgs {
    const float* w[2];
    int n;
    int layer[kMaxMfmaLayers], seg[kMaxMfmaLayers], blk0[kMaxMfmaLayers], which[kMaxMfmaLayers];
    int64_t cum[kMaxMfmaLayers + 1];  // fold: image elements; grad: rows x width
};

// Rewrites the image elements of the encoding segments' k blocks (W) / row blocks (W^T)
// from params, scaled: the elements mlp_pack_kernel writes there, through its index maps.
__global__ void mlp_fold_window_kernel(PackArgs a, WindowArgs f) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= f.cum[f.n]) return;
    int j = 0;
    while (g >= f.cum[j + 1]) ++j;
    const int l = f.layer[j], sg = f.seg[j], sb = a.seg_blk[l][sg];
    const int64_t img = (f.cum[j + 1] - f.cum[j]) / 2;  // NB x sb blocks of 1024 elements
    int64_t r = g - f.cum[j];
    const bool bwd = r >= img;
    if (bwd) r -= img;
    const int q = static_cast<int>(r / 1024);
    const int nb = q / sb, kb = f.blk0[j] + q % sb;  // output block, input block of the layer
    int64_t blk;
    if (!bwd)
        blk = a.prec != NR_PREC_FP32 ? static_cast<int64_t>(nb) * a.KB[l] + kb : static_cast<int64_t>(kb) * a.NB[l] + nb;
    else
        blk = static_cast<int64_t>(nb) * a.KB[l] + (kb - a.bwd_rot[l] + a.KB[l]) % a.KB[l];
    const PackLoc o = pack_locate(a, l, blk * 1024 + r % 1024, bwd);
    if (o.col < 0) return;  // padding stays zero
    const float v = a.params[a.w_off[l] + static_cast<int64_t>(o.row) * a.in[l] + o.col];
    pack_store(a, l, bwd, o.dst_e, v * window_scale(f.w[f.which[j]], o.col - a.seg_col0[l][sg]));
}

struct WindowGradArgs {
    float* g;
    int64_t w_off[kMaxMfmaLayers];
    int in[kMaxMfmaLayers], col0[kMaxMfmaLayers], width[kMaxMfmaLayers];
};

__global__ void window_grad_kernel(WindowGradArgs a, WindowArgs f) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= f.cum[f.n]) return;
    int j = 0;
    while (g >= f.cum[j + 1]) ++j;
    const float* w = f.w[f.which[j]];
    const int64_t r = g - f.cum[j];
    const int c = static_cast<int>(r % a.width[j]);
    if (!w || c < 3) return;
    a.g[a.w_off[j] + (r / a.width[j]) * a.in[j] + a.col0[j] + c] *= w[(c - 3) / 6];
}

// 16-bit dX-chain images (pk_bwdr): for layers l >= 1, A[i][k] = W[32 ob + k][hcol0 +
// 32 ib + i] with ib the hidden input block (row block), ob the output block (k
// block), row-block major: e = ((ib * NB + ob) * 2 + frag) * 512 + lane * 8 + el.
struct PackBwdrArgs {
    const float* params;
    char* packed;
    int prec;
    int l0, n_lin;                         // layers l0 .. n_lin-1
    int64_t w_off[kMaxMfmaLayers], pk[kMaxMfmaLayers];
    int in[kMaxMfmaLayers], NB[kMaxMfmaLayers], out[kMaxMfmaLayers], hcol0[kMaxMfmaLayers];
    int64_t cum[kMaxMfmaLayers + 1];       // element prefix over layers l0..
};

template <bool IDX>
__global__ void mlp_pack_bwdr_kernel(PackBwdrArgs a, PackIdx t) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= a.cum[a.n_lin]) return;
    int l = a.l0;
    while (g >= a.cum[l + 1]) ++l;
    const int64_t e = g - a.cum[l];
    const int el = static_cast<int>(e % 8), lane = static_cast<int>((e / 8) % 64);
    const int64_t frag = e / 512;
    const int sub = static_cast<int>(frag % 2);
    const int64_t blk = frag / 2;
    const int ob = static_cast<int>(blk % a.NB[l]), ib = static_cast<int>(blk / a.NB[l]);
    const int h = lane >> 5, i = lane & 31;
    const int kk = 16 * sub + 8 * (el >> 2) + 4 * h + (el & 3);
    const int row = 32 * ob + kk, col = a.hcol0[l] + 32 * ib + i;
    if constexpr (IDX) {
        if (row < a.out[l]) put_dst(t, 2, a.w_off[l] + static_cast<int64_t>(row) * a.in[l] + col, a.pk[l] + 2 * e, dst16(a.prec));
        return;
    }
    const float v = row < a.out[l] ? a.params[a.w_off[l] + static_cast<int64_t>(row) * a.in[l] + col] : 0.f;
    unsigned short* dst = reinterpret_cast<unsigned short*>(a.packed + a.pk[l]);
    dst[e] = a.prec == NR_PREC_FP16 ? __builtin_bit_cast(unsigned short, static_cast<_Float16>(v)) : bf16_bits(v);
}

// 16-bit forward images: the bias fragment that follows each row block's weights
// (bias_frag of bias[32 nb + lane] in lanes 0..31, zeros in 32..63).
struct PackBiasArgs {
    const float* params;
    char* packed;
    int prec;
    int n_lin;
    int64_t pk[kMaxMfmaLayers], b_off[kMaxMfmaLayers];
    int NB[kMaxMfmaLayers], KB[kMaxMfmaLayers], out[kMaxMfmaLayers];
};

template <int PREC, bool IDX>
__device__ void pack_bias_one(const PackBiasArgs& a, const PackIdx& t, int l, int nb, int lane) {
    const int row = 32 * nb + lane;
    if constexpr (IDX) {
        if (lane < 32 && row < a.out[l])
            put_dst(t, 0, a.b_off[l] + row,
                    a.pk[l] + (static_cast<int64_t>(nb) * (2 * a.KB[l] + 1) + 2 * a.KB[l]) * kFragBytes + 16 * lane,
                    PREC == NR_PREC_FP16 ? kDstFragF16 : kDstFragBf16);
        return;
    }
    const float b = (lane < 32 && row < a.out[l]) ? a.params[a.b_off[l] + row] : 0.f;
    const bf16x8 f = bias_frag<PREC>(b);
    char* dst = a.packed + a.pk[l] + (static_cast<int64_t>(nb) * (2 * a.KB[l] + 1) + 2 * a.KB[l]) * kFragBytes;
    reinterpret_cast<bf16x8*>(dst)[lane] = lane < 32 ? f : bf16x8{};
}

template <bool IDX>
__global__ void mlp_pack_bias_kernel(PackBiasArgs a, PackIdx t) {
    const int l = blockIdx.x / kMaxTrunk, nb = blockIdx.x % kMaxTrunk, lane = threadIdx.x;
    if (l >= a.n_lin || nb >= a.NB[l]) return;
    if (a.prec == NR_PREC_FP16)
        pack_bias_one<NR_PREC_FP16, IDX>(a, t, l, nb, lane);
    else
        pack_bias_one<NR_PREC_BF16, IDX>(a, t, l, nb, lane);
}

// Vector images: element idx of a vector of NB blocks <-> feature 32*(idx>>5) + acc_row(idx&15, (idx>>4)&1).
struct PackVecArgs {
    const float* params;
    char* packed;
    int nv;                                   // vectors: n_lin biases, w_sigma, 3 rows of W_rgb
    int64_t src[kMaxMfmaLayers + 8];          // float offset in params
    int len[kMaxMfmaLayers + 8];              // valid features
    int64_t dst[kMaxMfmaLayers + 8];          // byte offset in packed
    int cum[kMaxMfmaLayers + 9];              // image elements (NB*32) prefix
    int pair[kMaxMfmaLayers + 8];             // 1: pair image (PImg), 0: vector image (VImg)
    int slot[kMaxMfmaLayers + 8];             // destination-table slot (IDX mode)
};

template <bool IDX>
__global__ void mlp_pack_vec_kernel(PackVecArgs a, PackIdx t) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.cum[a.nv]) return;
    int v = 0;
    while (g >= a.cum[v + 1]) ++v;
    const int idx = g - a.cum[v];
    const int f = a.pair[v] ? 32 * (idx >> 5) + acc_row((idx >> 1) & 15, idx & 1)
                            : 32 * (idx >> 5) + acc_row(idx & 15, (idx >> 4) & 1);
    if constexpr (IDX) {
        if (f < a.len[v]) put_dst(t, a.slot[v], a.src[v] + f, a.dst[v] + 4 * static_cast<int64_t>(idx), kDstF32);
        return;
    }
    reinterpret_cast<float*>(a.packed + a.dst[v])[idx] = f < a.len[v] ? a.params[a.src[v] + f] : 0.f;
}

// ------------------------------------------------- fused optimizer step ----
// Adam over up to kMaxAdamSpans flat buffers (blockIdx.y = span), the clip
// coefficient from the span's clip-group partials (nr_sumsq_partials, summed in the
// fixed block order by every block), and the packed images refreshed through the
// span's destination table: nr_mlp_pack's four kernels are not run after the step.
// (AdamMultiArgs: mlp_launch.hpp)
__device__ __forceinline__ void put_image(char* packed, uint32_t e, float p) {
    char* q = packed + (e & 0x1fffffffu);
    switch (e >> 29) {
        case kDstF32: *reinterpret_cast<float*>(q) = p; break;
        case kDstBf16: *reinterpret_cast<unsigned short*>(q) = bf16_bits(p); break;
        case kDstF16: *reinterpret_cast<unsigned short*>(q) = __builtin_bit_cast(unsigned short, static_cast<_Float16>(p)); break;
        case kDstFragBf16: *reinterpret_cast<bf16x8*>(q) = bias_frag<NR_PREC_BF16>(p); break;
        case kDstFragF16: *reinterpret_cast<bf16x8*>(q) = bias_frag<NR_PREC_FP16>(p); break;
        default: break;
    }
}

__global__ void __launch_bounds__(kSumsqThreads) adam_multi_kernel(AdamMultiArgs a) {
    const AdamSpanDev& s = a.s[blockIdx.y];
    const float step_size = a.sched ? a.sched[0] : a.step_size, bc2_sqrt = a.sched ? a.sched[1] : a.bc2_sqrt;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t t0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t n = s.n;
    // 16-B accesses when every buffer (and the table's slot rows) allows them
    const int64_t n4 = (n % 4 == 0) ? n / 4 : 0;
    float4 P, G, M, V;
    u32x4 E[kPackSlots];
    auto load = [&](int64_t i) {
        P = reinterpret_cast<const float4*>(s.p)[i];
        G = reinterpret_cast<const float4*>(s.g)[i];
        M = reinterpret_cast<const float4*>(s.m)[i];
        V = reinterpret_cast<const float4*>(s.v)[i];
        if (s.table)
#pragma unroll
            for (int sl = 0; sl < kPackSlots; ++sl) E[sl] = reinterpret_cast<const u32x4*>(s.table + sl * n)[i];
    };
    // the first element's loads go out before the clip coefficient's 256 partials are
    // summed (per wave, no barrier: the grid is one element per thread at NeRF sizes)
    if (t0 < n4) load(t0);
    const float coef = s.partials ? clip_coef(wave_sum_fixed(s.partials), s.max_norm) : 1.0f;
    for (int64_t i = t0; i < n4; i += stride) {
        if (i != t0) load(i);
        adam_one(P.x, G.x, M.x, V.x, coef, a.omb1, a.b2, a.omb2, step_size, bc2_sqrt, a.eps);
        adam_one(P.y, G.y, M.y, V.y, coef, a.omb1, a.b2, a.omb2, step_size, bc2_sqrt, a.eps);
        adam_one(P.z, G.z, M.z, V.z, coef, a.omb1, a.b2, a.omb2, step_size, bc2_sqrt, a.eps);
        adam_one(P.w, G.w, M.w, V.w, coef, a.omb1, a.b2, a.omb2, step_size, bc2_sqrt, a.eps);
        reinterpret_cast<float4*>(s.p)[i] = P;
        reinterpret_cast<float4*>(s.g)[i] = G;
        reinterpret_cast<float4*>(s.m)[i] = M;
        reinterpret_cast<float4*>(s.v)[i] = V;
        if (s.table) {
#pragma unroll
            for (int sl = 0; sl < kPackSlots; ++sl) {
                put_image(s.packed, E[sl].x, P.x);
                put_image(s.packed, E[sl].y, P.y);
                put_image(s.packed, E[sl].z, P.z);
                put_image(s.packed, E[sl].w, P.w);
            }
        }
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        float P1 = s.p[i], G1 = s.g[i], M1 = s.m[i], V1 = s.v[i];
        adam_one(P1, G1, M1, V1, coef, a.omb1, a.b2, a.omb2, step_size, bc2_sqrt, a.eps);
        s.p[i] = P1;
        s.g[i] = G1;
        s.m[i] = M1;
        s.v[i] = V1;
        if (s.table)
#pragma unroll
            for (int sl = 0; sl < kPackSlots; ++sl) put_image(s.packed, s.table[sl * n + i], P1);
    }
}

namespace {

PackArgs pack_args(const MlpPlan& p, const float* params, void* packed) {
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.params = params;
    a.packed = static_cast<char*>(packed);
    a.n_lin = p.n_lin;
    a.prec = p.prec;
    a.cum[0] = 0;
    for (int l = 0; l < p.n_lin; ++l) {
        const LinearDesc& d = p.lin[l];
        a.w_off[l] = d.w_off;
        a.in[l] = d.in;
        a.NB[l] = d.NB;
        a.KB[l] = d.KB;
        a.nseg[l] = d.nseg;
        for (int s = 0; s < d.nseg; ++s) {
            a.seg_col0[l][s] = d.seg[s].col0;
            a.seg_w[l][s] = d.seg[s].width;
            a.seg_blk[l][s] = d.seg[s].blocks;
        }
        a.pk[l] = d.pk_fwd;
        a.pkb[l] = d.pk_bwd;
        a.bwd_rot[l] = (l > 0 && l < p.n_layers && is_skip(p, l - 1)) ? d.seg[0].blocks : 0;
        const int64_t elems = static_cast<int64_t>(d.NB) * d.KB * 1024;  // 32x32 elements per block
        a.cum[l + 1] = a.cum[l] + 2 * elems;
    }
    return a;
}

// the plan's encoding segments (WindowArgs without its element counts)
WindowArgs window_segments(const MlpPlan& p, const float* w_pos, const float* w_dir) {
    WindowArgs f;
    std::memset(&f, 0, sizeof(f));
    f.w[0] = w_pos;
    f.w[1] = w_dir;
    auto add = [&](int l, int sg, int which) {
        f.layer[f.n] = l;
        f.seg[f.n] = sg;
        f.which[f.n] = which;
        for (int s = 0; s < sg; ++s) f.blk0[f.n] += p.lin[l].seg[s].blocks;
        ++f.n;
    };
    for (int i = 0; i < p.n_layers; ++i)
        if (i == 0 || is_skip(p, i - 1)) add(i, 0, 0);
    if (p.use_vd) add(p.n_layers + 1, 1, 1);
    return f;
}

// nr_mlp_pack's four kernels; IDX: their index mode, filling the destination table
template <bool IDX>
int launch_pack_t(const MlpPlan& p, const float* params, void* packed, PackIdx t, hipStream_t s) {
    const char* what = IDX ? "nr_mlp_pack_table" : "nr_mlp_pack";
    const PackArgs a = pack_args(p, params, packed);
    const int64_t total = a.cum[p.n_lin];
    hipLaunchKernelGGL(mlp_pack_kernel<IDX>, dim3(static_cast<unsigned>(ceil_div_ll(total, 256))), dim3(256), 0, s, a, t);
    NR_LAUNCH_CHECK(what);
    if (p.prec != NR_PREC_FP32) {
        PackBiasArgs pb;
        std::memset(&pb, 0, sizeof(pb));
        pb.params = params;
        pb.packed = static_cast<char*>(packed);
        pb.prec = p.prec;
        pb.n_lin = p.n_lin;
        for (int l = 0; l < p.n_lin; ++l) {
            pb.pk[l] = p.lin[l].pk_fwd;
            pb.b_off[l] = p.lin[l].b_off;
            pb.NB[l] = p.lin[l].NB;
            pb.KB[l] = p.lin[l].KB;
            pb.out[l] = p.lin[l].out;
        }
        hipLaunchKernelGGL(mlp_pack_bias_kernel<IDX>, dim3(p.n_lin * kMaxTrunk), dim3(64), 0, s, pb, t);
        NR_LAUNCH_CHECK(what);
        if (p.n_lin > 1) {
            PackBwdrArgs pr;
            std::memset(&pr, 0, sizeof(pr));
            pr.params = params;
            pr.packed = static_cast<char*>(packed);
            pr.prec = p.prec;
            pr.l0 = 1;
            pr.n_lin = p.n_lin;
            pr.cum[1] = 0;
            for (int l = 1; l < p.n_lin; ++l) {
                const LinearDesc& d = p.lin[l];
                pr.w_off[l] = d.w_off;
                pr.pk[l] = d.pk_bwdr;
                pr.in[l] = d.in;
                pr.NB[l] = d.NB;
                pr.out[l] = d.out;
                // the hidden input columns: after x_enc in a skip layer (cat([x_enc, h])), first otherwise
                pr.hcol0[l] = (l < p.n_layers && is_skip(p, l - 1)) ? p.pos_dim : 0;
                pr.cum[l + 1] = pr.cum[l] + static_cast<int64_t>(kHB) * d.NB * 1024;
            }
            const int64_t tot = pr.cum[p.n_lin];
            hipLaunchKernelGGL(mlp_pack_bwdr_kernel<IDX>, dim3(static_cast<unsigned>(ceil_div_ll(tot, 256))), dim3(256),
                               0, s, pr, t);
            NR_LAUNCH_CHECK(what);
        }
    }
    PackVecArgs v;
    std::memset(&v, 0, sizeof(v));
    v.params = params;
    v.packed = static_cast<char*>(packed);
    auto add_vec = [&](int64_t src, int len, int64_t dst, int nblk, int pair, int slot) {
        v.pair[v.nv] = pair;
        v.slot[v.nv] = slot;
        v.src[v.nv] = src;
        v.len[v.nv] = len;
        v.dst[v.nv] = dst;
        v.cum[v.nv + 1] = v.cum[v.nv] + nblk * 32;
        v.nv++;
    };
    // table slots: biases 1 (slot 0 holds their 16-bit fragment), the head weights'
    // pair images 0 and their vector images 1
    for (int l = 0; l < p.n_lin; ++l) add_vec(p.lin[l].b_off, p.lin[l].out, p.lin[l].vb, p.lin[l].NB, 0, 1);
    add_vec(p.sig_w, kHidden, p.vsig, kHB, 1, 0);
    for (int c = 0; c < 3; ++c)
        add_vec(p.rgb_w + c * (kHidden / 2), kHidden / 2, p.vrgb + c * (kHidden / 2) * 4, kHB / 2, 1, 0);
    add_vec(p.sig_w, kHidden, p.vhead, kHB, 0, 1);
    for (int c = 0; c < 3; ++c)
        add_vec(p.rgb_w + c * (kHidden / 2), kHidden / 2, p.vhead + 1024 + c * (kHidden / 2) * 4, kHB / 2, 0, 1);
    hipLaunchKernelGGL(mlp_pack_vec_kernel<IDX>, dim3(ceil_div(v.cum[v.nv], 256)), dim3(256), 0, s, v, t);
    NR_LAUNCH_CHECK(what);
    return NR_OK;
}

}  // namespace

int launch_pack(const MlpPlan& p, const float* params, void* packed, PackIdx t, bool idx, hipStream_t s) {
    return idx ? launch_pack_t<true>(p, params, packed, t, s) : launch_pack_t<false>(p, params, packed, t, s);
}

int launch_fold_window(const MlpPlan& p, const float* params, void* packed, const float* w_pos, const float* w_dir,
                       hipStream_t s) {
    const PackArgs a = pack_args(p, params, packed);
    WindowArgs f = window_segments(p, w_pos, w_dir);
    for (int j = 0; j < f.n; ++j) {
        const LinearDesc& d = p.lin[f.layer[j]];
        f.cum[j + 1] = f.cum[j] + 2 * static_cast<int64_t>(d.NB) * d.seg[f.seg[j]].blocks * 1024;
    }
    if (f.cum[f.n] == 0) return NR_OK;
    hipLaunchKernelGGL(mlp_fold_window_kernel, dim3(static_cast<unsigned>(ceil_div_ll(f.cum[f.n], 256))), dim3(256), 0,
                       s, a, f);
    return check_launch("nr_mlp_fold_window");
}

int launch_window_grad(const MlpPlan& p, const float* w_pos, const float* w_dir, float* g_params, hipStream_t s) {
    WindowArgs f = window_segments(p, w_pos, w_dir);
    WindowGradArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = g_params;
    for (int j = 0; j < f.n; ++j) {
        const LinearDesc& d = p.lin[f.layer[j]];
        a.w_off[j] = d.w_off;
        a.in[j] = d.in;
        a.col0[j] = d.seg[f.seg[j]].col0;
        a.width[j] = d.seg[f.seg[j]].width;
        f.cum[j + 1] = f.cum[j] + static_cast<int64_t>(d.out) * a.width[j];
    }
    if (f.cum[f.n] == 0) return NR_OK;
    hipLaunchKernelGGL(window_grad_kernel, dim3(static_cast<unsigned>(ceil_div_ll(f.cum[f.n], 256))), dim3(256), 0, s,
                       a, f);
    return check_launch("nr_mlp_window_grad");
}

int launch_adam_multi(const AdamMultiArgs& a, int grid, int nspan, hipStream_t s) {
    hipLaunchKernelGGL(adam_multi_kernel, dim3(grid, nspan), dim3(kSumsqThreads), 0, s, a);
    return check_launch("nr_adam_multi");
}

}  // namespace nr
